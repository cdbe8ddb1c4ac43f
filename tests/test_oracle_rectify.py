"""The CPU restatement of the frame rectification (tests/rectify_oracle.c, the contract of a3_rectify_frames in include/aruco3_hip.h)
against a float64 numpy reference, on the identity, and end to end: frames rendered through a lens, rectified by the oracle, put the
detector's corners where the ideal pinhole camera sees them.  No GPU: the device kernel is held to the same oracle byte for byte in
tests/test_gpu_rectify.py."""
import numpy as np
import pytest

from tests import lens_oracle as lo
from tests import rectify_oracle as ro


def _noise(h=ro.SRC_SIZE[1], w=ro.SRC_SIZE[0], c=None, seed=3):
    shape = (h, w) if c is None else (h, w, c)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _reference64(img, K, k, new_K, new_size, R):
    """the contract in float64 -> (blended value, inside, excluded) per output pixel; excluded: (u, v) within 0.01 px of the source
    border, not finite, or |Wz| < 1e-6 -- where f32 and f64 may legitimately disagree about `inside`"""
    h, w = img.shape
    fx, fy, cx, cy = K
    nfx, nfy, ncx, ncy = new_K
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    j, i = np.meshgrid(np.arange(new_size[0], dtype=np.float64), np.arange(new_size[1], dtype=np.float64))
    P = np.stack([(j - ncx) / nfx, (i - ncy) / nfy, np.ones_like(j)], -1) @ R   # (R^T applied to each column vector)
    with np.errstate(all="ignore"):
        x, y = P[..., 0] / P[..., 2], P[..., 1] / P[..., 2]
        r2 = x * x + y * y
        rad = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
        u = (x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)) * fx + cx
        v = (y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y) * fy + cy
        finite = np.isfinite(u) & np.isfinite(v)
        inside = (P[..., 2] > 0) & finite & (u >= 0) & (v >= 0) & (u <= w - 1) & (v <= h - 1)
        margin = np.minimum.reduce([np.abs(u), np.abs(v), np.abs(u - (w - 1)), np.abs(v - (h - 1))])
        excluded = ~finite | (margin < 1e-2) | (np.abs(P[..., 2]) < 1e-6)
    uu, vv = np.where(inside, u, 0.0), np.where(inside, v, 0.0)
    x0, y0 = np.floor(uu).astype(int), np.floor(vv).astype(int)
    ax, ay = uu - x0, vv - y0
    x1, y1 = np.minimum(x0 + 1, w - 1), np.minimum(y0 + 1, h - 1)
    s = img.astype(np.float64)
    val = (1 - ay) * ((1 - ax) * s[y0, x0] + ax * s[y0, x1]) + ay * ((1 - ax) * s[y1, x0] + ax * s[y1, x1])
    return val, inside, excluded


@pytest.mark.parametrize("view", list(ro.VIEWS))
@pytest.mark.parametrize("coeffs", list(lo.COEFFS))
def test_oracle_against_float64(coeffs, view):
    """`inside` agrees exactly and every byte lies within one grey level of the float64 blend, away from the source border (at most
    0.1 % of the pixels may be that close: a condition of the comparison, not a tolerance)"""
    img = _noise()
    new_K, size, deg = ro.VIEWS[view]
    R = ro.rot_y(deg)
    got, inside = ro.rectify(img, ro.SRC_K, lo.COEFFS[coeffs], new_K, size, R, fill=77, with_inside=True)
    got = got[0, :, :, 0]
    val, inside64, excluded = _reference64(img, ro.SRC_K, lo.COEFFS[coeffs], new_K, size, R)
    print(f"{coeffs} {view}: inside {inside64.mean():.3f}, excluded {excluded.mean():.5f}")
    assert excluded.mean() <= 1e-3
    keep = ~excluded
    assert np.array_equal(inside[keep], inside64[keep])
    assert np.all(got[~inside] == 77)
    m = keep & inside64
    if m.any():
        err = np.abs(got[m].astype(np.float64) - val[m]).max()
        print(f"  worst |out - float64| {err:.3f}")
        assert err <= 1.0
    if view == "rot80":
        assert (~inside64).mean() > 0.5   # (rays with Wz <= 0 included)


@pytest.mark.parametrize("c", [None, 3, 4])
def test_identity(c):
    """no lens, R = I, fx = fy = 256 and an integer principal point: the normalisation round-trips exactly, so the output is the input
    byte for byte (L8, RGB8, and four bytes per pixel: RGBA8 and BGRA8 are the same bytes to this call)"""
    h, w = 61, 97
    img = _noise(h, w, c, seed=5)
    K = (256.0, 256.0, 40.0, 23.0)
    for coeffs in (None, np.zeros(8)):
        out, inside = ro.rectify(img, K, coeffs, with_inside=True)
        assert inside.all()
        assert np.array_equal(out[0].reshape(img.shape), img)


def test_strides_frames_and_padding():
    """strided source and destination, several frames: rows land where the strides say, and no padding byte is written"""
    rng = np.random.default_rng(9)
    n, bpp, (w, h) = 3, 3, (45, 31)
    frames = rng.integers(0, 256, (n, h, w, bpp), dtype=np.uint8)
    K, k = (60.0, 60.0, 22.0, 15.0), lo.COEFFS["webcam5"]
    want = ro.rectify(frames, K, k, fill=9)
    srow, sframe = w * bpp + 7, (w * bpp + 7) * h + 11
    src = np.zeros(5 + sframe * n, np.uint8)
    for f in range(n):
        for y in range(h):
            src[5 + f * sframe + y * srow: 5 + f * sframe + y * srow + w * bpp] = frames[f, y].reshape(-1)
    drow, dframe = w * bpp + 3, (w * bpp + 3) * h + 13
    dst = np.full(dframe * n, 0xA5, np.uint8)
    ro.rectify_raw(src[5:], w, h, bpp, srow, sframe, n, K, k, K, np.eye(3), 9, dst, w, h, drow, dframe)
    written = np.zeros(dst.size, bool)
    for f in range(n):
        for y in range(h):
            o = f * dframe + y * drow
            assert np.array_equal(dst[o: o + w * bpp], want[f, y].reshape(-1))
            written[o: o + w * bpp] = True
    assert np.all(dst[~written] == 0xA5)


def test_end_to_end_accuracy_through_a_lens():
    """5 x 7 grid board at 1280 x 720 rendered on the host through the WEBCAM lens (the scenes of test_accuracy_through_a_lens):
    the oracle detector's integer corners against the ideal pinhole projections, on the raw frames and on the oracle-rectified
    ones (same fx fy cx cy, no coefficients).  Integer corners sit about a pixel inside the border by construction.
    Measured: raw median 12.95 px, rectified 1.06 px."""
    from aruco3_amd import ARDictionary
    from aruco3_amd.board import GridBoard
    from oracle import a3oracle
    from tests import board_util as bu
    from tests import lens_util as lu

    d = ARDictionary.new_from_named_dict("ARUCO")
    board = GridBoard(5, 7, 30.0, 6.0, first_id=10)
    codes = np.asarray(d.code_list, dtype=np.uint64)
    cfg = a3oracle.Config.default()
    cfg.min_corner_separation_factor = bu.MIN_CORNER_SEPARATION_FACTOR   # (the detector configuration of bu.config())
    rng = np.random.default_rng(11)
    errs = {"raw": [], "rectified": []}
    for off in ((-300.0, -90.0), (290.0, 90.0), (-280.0, 100.0), (300.0, -90.0)):
        R, t = bu.board_pose_facing(board, rng.uniform(20, 40), rng.uniform(0, 360), rng.uniform(-20, 20), rng.uniform(480, 520), off, K=lu.K720)
        raw = lu.render(board, d, R, t)
        rect = ro.rectify(raw, lu.K720, lu.WEBCAM)[0, :, :, 0]
        truth = bu.project(board, R, t, lu.K720)
        for name, img in (("raw", raw), ("rectified", rect)):
            found = 0
            for m in a3oracle.detect(img, codes, d.num_bits, d._tau, cfg, keep_debug=False)["markers"]:
                slot = np.nonzero(board.ids == m["id"])[0]
                if slot.size:
                    found += 1
                    errs[name].append(np.linalg.norm(np.asarray(m["corners"], np.float64).reshape(4, 2) - truth[slot[0]], axis=1))
            print(f"{name}: {found} board markers")
            assert found >= 15
    med = {k: float(np.median(np.concatenate(v))) for k, v in errs.items()}
    print(f"median integer-corner error: raw {med['raw']:.2f} px, rectified {med['rectified']:.2f} px")
    assert med["rectified"] < 1.5
    assert med["rectified"] < med["raw"] / 5.0


def test_no_device_fails_loudly():
    """without a GPU rectify_frames raises, it never falls back to host arithmetic"""
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import aruco3_amd
    from aruco3_amd import CameraIntrinsics, _lib

    with pytest.raises(_lib.A3Error) as e:
        aruco3_amd.rectify_frames(np.zeros((8, 8, 3), np.uint8), CameraIntrinsics(8, 8, 10.0, 10.0))
    assert e.value.code == _lib.ERR_NO_DEVICE
