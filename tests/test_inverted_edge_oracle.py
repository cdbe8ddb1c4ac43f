"""The edge fit restated with a polarity per quad (tests/inverted_edge_oracle.c) against the restatement the kernel has been held to so
far (tests/edge_refine_oracle.c), without a GPU: polarity 0 is the same function to the bit on every scene of tests/edge_refine_cases.py,
and polarity 1 on the complemented frame finds the corners polarity 0 finds on the frame as drawn, up to the rounding of the bilinear
samples of 255 - I."""
import numpy as np
import pytest

from tests import edge_refine_cases as ec
from tests import edge_refine_oracle as ero
from tests import inverted_edge_oracle as ieo

# Largest |difference| in pixels, over every coordinate of every scene, between polarity 1 on 255 - frame and the existing oracle on
# the frame: measured 7.63e-06 (2^-17: one f32 ulp of a coordinate between 64 and 128, in the scenes "slanted" and "one_pass"; 0 in the
# other seven).  The two computations differ only in the rounding of the bilinear samples of 255 - I, which are 255 - S up to the last
# bit of each product.  The bound is four times the measured value.
MEASURED_PX = 2.0 ** -17
BOUND_PX = 4.0 * MEASURED_PX


@pytest.mark.parametrize("name", sorted(ec.scenes()))
def test_polarity_zero_is_the_existing_oracle_bit_for_bit(name):
    grey, quads, cfg, cell = ec.scenes()[name]
    want = ero.refine_quads(grey, quads, cfg, cell)
    assert ieo.refine_quads(grey, quads, cfg, cell).tobytes() == want.tobytes()
    assert ieo.refine_quads(grey, quads, cfg, cell, np.zeros(len(quads), np.uint32)).tobytes() == want.tobytes()


def test_polarity_one_on_the_complement_finds_the_corners_of_the_frame_as_drawn():
    worst, moved = 0.0, 0
    for name, (grey, quads, cfg, cell) in sorted(ec.scenes().items()):
        want = ero.refine_quads(grey, quads, cfg, cell)
        got = ieo.refine_quads(255 - grey, quads, cfg, cell, np.ones(len(quads), np.uint32))
        d = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print(f"{name}: largest difference {d:.3g} px")
        worst = max(worst, d)
        moved += int((want != np.asarray(quads, np.float32).reshape(want.shape)).any())
    print(f"largest difference over all scenes {worst:.3g} px (bound {BOUND_PX:.3g})")
    assert moved >= 3          # (scenes in which the fit moves a corner at all)
    assert worst <= BOUND_PX


def test_the_wrong_polarity_finds_no_edge():
    """the polarity filter at work: a dark quad read as bright inside has no live station on its own sides and reverts"""
    grey, quads, cfg, cell = ec.scenes()["slanted"]
    start = np.asarray(quads, np.float32).reshape(-1, 4, 2)
    got = ieo.refine_quads(grey, quads, cfg, cell, np.ones(len(quads), np.uint32))
    assert got.tobytes() == start.tobytes()
    got = ieo.refine_quads(255 - grey, quads, cfg, cell, None)
    assert got.tobytes() == start.tobytes()


def test_mixed_polarities_in_one_call():
    grey, quads, cfg, cell = ec.scenes()["slanted"]
    both = np.concatenate([quads, quads])
    pol = np.array([0] * len(quads) + [1] * len(quads), np.uint32)
    got = ieo.refine_quads(grey, both, cfg, None if cell is None else np.concatenate([cell, cell]), pol)
    assert got[: len(quads)].tobytes() == ero.refine_quads(grey, quads, cfg, cell).tobytes()
    assert got[len(quads):].tobytes() == np.asarray(quads, np.float32).reshape(-1, 4, 2).tobytes()
