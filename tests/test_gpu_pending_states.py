"""The pending per-dart states of the contour stage on the device: a dense batch whose global doubling rounds are cut short on purpose
(a3_debug_set_jump_rounds).  Its entry states have not converged when k_jump_finalize resolves the pending states from them, and
every sweep after it must see that without writing outside its tables: the library notices the short launch and re-runs the batch
with all rounds.  GPU only."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_too_few_global_rounds_rerun_and_match_the_oracle(dicts, oracle):
    from aruco3_amd import _lib
    from tests.test_gpu_shard_taps import _compare_contours, _detect_host, _detector

    rng = np.random.default_rng(2026)
    frames = rng.integers(0, 256, size=(2, 360, 480), dtype=np.uint8)   # noise: a dense graph, entries beyond k_entry_frame's LDS
    det = _detector(dicts, "ARUCO_DEFAULT")
    L = _lib.load()
    ctx, _, _ = _detect_host(det, frames[..., None], taps=True)   # a frame's entries overflow k_entry_frame: the global rounds take over
    ctx, ref_markers, ref_per = _detect_host(det, frames[..., None], taps=True)
    full = ctx.stats()
    assert full["jump_rounds"] > 1, full
    assert L.a3_debug_set_jump_rounds(1) == 0
    try:
        ctx, n = _compare_contours(det, oracle, frames)   # (every border of every frame against the oracle)
        st = ctx.stats()
        ctx, markers, per = _detect_host(det, frames[..., None], taps=False)
        st2 = ctx.stats()
    finally:
        assert L.a3_debug_set_jump_rounds(0) == 0
    assert n > 1000
    # the short launch was seen and the batch run again, with all rounds
    assert st["reruns"] >= full["reruns"] + 1 and st2["reruns"] >= 1, (full, st, st2)
    assert np.array_equal(markers, ref_markers) and np.array_equal(per, ref_per)
    assert L.a3_last_error(ctx.handle) in (None, b"")                    # no error left behind
