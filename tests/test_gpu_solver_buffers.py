"""The solver entry points share one set of device buffers per context (solve_in / solve_scratch / solve_big / solve_out): on ONE context
the five of them, one after the other and then again after a call that made the buffers grow, must return exactly the bytes that the
same call returns on a fresh context -- nothing of what another family staged, computed or left behind may show."""
import numpy as np
import pytest

from tests import calib_util as cu
from tests import fisheye_calib_util as fu
from tests import handeye_util as hu
from tests import map_util as mu
from tests import rig_util as ru

pytestmark = pytest.mark.gpu


def _context():
    import torch

    from aruco3_amd import _lib

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1)


def _two_cameras(n_views):
    ps = [cu.problem("charuco", n_views, seed=70 + k, coeffs=cu.WEBCAM) for k in range(2)]
    offsets = np.concatenate([ps[0]["offsets"], ps[1]["offsets"][1:] + ps[0]["offsets"][-1]]).astype(np.uint32)
    cams = cu.cameras([dict(size=p["size"], first_view=n_views * k, n_views=n_views) for k, p in enumerate(ps)])
    return cams, offsets, np.concatenate([p["obj"] for p in ps]), np.concatenate([p["img"] for p in ps])


def test_one_context_serves_every_solver_like_a_fresh_one():
    from aruco3_amd import _lib

    pc = cu.problem("charuco", 3, seed=71, coeffs=cu.WEBCAM)
    pf = fu.problem("charuco", 3, seed=72, coeffs=fu.MILD)
    cameras = ("calibrate_cameras", (cu.one_camera(pc), pc["offsets"], pc["obj"], pc["img"]))
    rigs = ("calibrate_rigs", ru.pack([ru.make_rig(2, 2, seed=73)]))
    hand_eyes = ("calibrate_hand_eyes", hu.pack([hu.make_problem(F=3, seed=74)]))
    maps = ("build_marker_maps", mu.pack([mu.make_map(2, 2, seed=75)]))
    fisheye = ("calibrate_fisheye_cameras", (fu.one_camera(pf), pf["offsets"], pf["obj"], pf["img"]))
    larger = ("calibrate_cameras", _two_cameras(5))   # more input and more output than anything before it: the buffers grow
    # the camera owns views 0 and 1 of the three: the last one belongs to nobody and comes back zero
    unowned = ("calibrate_cameras", (cu.cameras([dict(size=pc["size"], first_view=0, n_views=2)]), pc["offsets"], pc["obj"], pc["img"]))

    def call(ctx, method, args):
        return [bytes(a) for a in getattr(ctx, method)(*args)]

    shared = _context()
    try:
        for step, (method, args) in enumerate((cameras, rigs, hand_eyes, maps, fisheye, larger, rigs, unowned)):
            got = call(shared, method, args)
            fresh = _context()
            try:
                want = call(fresh, method, args)
            finally:
                fresh.close()
            assert got == want, (step, method, [g == w for g, w in zip(got, want)])
        view = len(bytes(_lib.CalibView()))
        assert len(got[1]) == 3 * view and got[1][2 * view:] == bytes(view) and got[1][:view] != bytes(view)
    finally:
        shared.close()
