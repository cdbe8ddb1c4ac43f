"""The decode stage's frame sampler (sample_issue / sample_finish / pair_from / luma_px in csrc/k_decode.hip): frames, buffer layouts,
quads and -- per sample -- the case the sampler is expected to take.  Pure numpy; tests/test_sampler_cases.py checks on any machine
that every case group reaches the cases it claims, tests/test_gpu_decode_sampler.py runs the groups on the device.

The sampler has three cases per sample (TapLoad.mode):
  OUTSIDE  the bilinear footprint leaves the frame: the sample is 0 (mode 0)
  TAIL     inside, but a 12-byte read at the bottom tap would run past the frame's last byte: byte loads (mode 2)
  WIDE     inside otherwise: two 12-byte reads from the frame base rounded down to 4 bytes (mode 1)
and two offset widths: 32 bits while frame_bytes < 0xFFFFFFE0 and row_stride < 2^24, 64 bits beyond."""
import numpy as np

S = 49                       # homography_sample_size of the default configuration
OUTSIDE, TAIL, WIDE = 0, 1, 2
MODE_NAMES = ("outside", "tail", "wide")
BPP = {"L8": 1, "RGB8": 3, "RGBA8": 4, "BGRA8": 4}
DICTIONARY = "ARUCO_DEFAULT"


# ------------------------------------------------------------------------------------------------------------------
# frames and layouts
# ------------------------------------------------------------------------------------------------------------------
def noise_frames(seed, n, h, w, fmt):
    """uniform noise, every channel drawn on its own: a tap one byte, one channel or one pixel off changes the grey value"""
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, BPP[fmt]), dtype=np.uint8)


def lay(frames, lead=0, pad=0, gap=0, seed=1):
    """frames [n, h, w, c] laid into a buffer of OTHER noise: the first frame starts at byte `lead`, a row takes w * c + pad bytes,
    a frame h rows + gap bytes -> (buffer, row_stride, frame_stride)"""
    n, h, w, c = frames.shape
    row_stride = w * c + pad
    frame_stride = h * row_stride + gap
    buf = np.random.default_rng(1000 + seed).integers(0, 256, lead + n * frame_stride + 16, dtype=np.uint8)
    laid(buf, lead, row_stride, frame_stride, n, h, w, c)[...] = frames
    return buf, row_stride, frame_stride


def laid(buf, lead, row_stride, frame_stride, n, h, w, c):
    """the [n, h, w, c] view of the frames inside such a buffer"""
    return np.lib.stride_tricks.as_strided(buf[lead:], (n, h, w, c), (frame_stride, row_stride, c, 1))


def for_oracle(frame, fmt):
    """one frame [h, w, c] (a view will do) as the oracle takes it: [h, w] for L8, channels in R, G, B(, A) order otherwise"""
    if fmt == "L8":
        return frame[:, :, 0]
    if fmt == "BGRA8":
        return np.ascontiguousarray(frame[:, :, [2, 1, 0, 3]])
    return frame


def frame_bytes(w, h, bpp, row_stride):
    return (h - 1) * row_stride + w * bpp


def offsets_are_64_bit(w, h, bpp, row_stride):
    """k_decode's `off32` negated: which instantiation of sample_issue a layout runs"""
    return not (frame_bytes(w, h, bpp, row_stride) < 0xFFFFFFE0 and row_stride < (1 << 24))


# ------------------------------------------------------------------------------------------------------------------
# quads
# ------------------------------------------------------------------------------------------------------------------
def quad_set(w, h):
    """quads for a frame of at least 40 x 20: hugging every edge and corner (coordinates 0 and w - 1 / h - 1), reaching past the frame (up
    to w + 20, h + 20), a small one (~8 px), the whole frame, a rotated and a strongly perspective one, and one whose interior is the
    frame's last pixels (the last 12 bytes).  Corners are pairwise far enough apart for discard_too_near to keep them all."""
    assert w >= 40 and h >= 20
    u = max(4, min(w, h) // 5)
    e = u + 3
    cx, cy = w // 2, h // 2
    r = 0.35 * min(w, h)
    ang = np.deg2rad(25.0 + 90.0 * np.arange(4))
    rot = [(int(round(cx + r * np.cos(a))), int(round(cy + r * np.sin(a)))) for a in ang]
    box = lambda x0, y0, x1, y1: [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    q = [
        box(0, 2 * u, e, 2 * u + e),                          # left edge
        box(2 * u, 0, 2 * u + e, e),                          # top edge
        box(w - 1 - e, u, w - 1, u + e),                      # right edge
        box(3 * u, h - 1 - e, 3 * u + e, h - 1),              # bottom edge
        box(0, 0, u, u), box(w - 1 - u, 0, w - 1, u),         # the four corners
        box(w - 1 - u, h - 1 - u, w - 1, h - 1), box(0, h - 1 - u, u, h - 1),
        [(w - 2 * u, h - 2 * u), (w + 20, h - u), (w + 12, h + 20), (w - 3 * u, h + 8)],      # past the right and bottom edges
        [(w - u, 0), (w + 20, 2), (w + 18, u + 4), (w - u - 2, u)],                           # past the right edge, at the top
        [(cx - 4, cy - 3), (cx + 4, cy - 4), (cx + 5, cy + 4), (cx - 3, cy + 5)],             # small
        box(0, 0, w - 1, h - 1),                                                              # the whole frame
        rot,                                                                                  # rotated
        [(1, 2), (w - 2, 4), (cx + u // 2 + 1, h - 3), (cx - u // 2, h - 4)],                 # strongly perspective
        [(w - 1, h - 1), (w - 6, h - 1), (w - 6, h - 6), (w - 1, h - 6)],                     # the frame's last pixels (listed from the far corner)
    ]
    return np.asarray(q, dtype=np.uint32)


# frames too small for quad_set: (format, w, h, quads, modes the case reaches)
TINY_CASES = [
    ("L8", 5, 3, [[(0, 0), (4, 0), (4, 2), (0, 2)], [(1, 0), (3, 0), (3, 2), (1, 2)], [(0, 0), (24, 0), (24, 22), (0, 22)]], (OUTSIDE, TAIL)),   # 15 bytes: `tiny`
    ("L8", 4, 4, [[(0, 0), (3, 0), (3, 3), (0, 3)], [(0, 0), (2, 0), (2, 2), (0, 2)], [(1, 1), (23, 1), (23, 23), (1, 23)]], (OUTSIDE, TAIL, WIDE)),   # 16 bytes: one wide offset
    ("RGB8", 2, 2, [[(0, 0), (1, 0), (1, 1), (0, 1)], [(0, 0), (21, 0), (21, 21), (0, 21)]], (OUTSIDE, TAIL)),
    ("RGBA8", 2, 2, [[(0, 0), (1, 0), (1, 1), (0, 1)], [(0, 0), (21, 0), (21, 21), (0, 21)]], (OUTSIDE, TAIL)),
    ("L8", 16, 1, [[(0, 0), (15, 0), (15, 10), (0, 10)], [(2, 0), (9, 0), (9, 20), (2, 20)]], (OUTSIDE,)),      # one row: no sample has a bottom tap
    ("RGBA8", 1, 3, [[(0, 0), (10, 0), (10, 2), (0, 2)], [(0, 0), (20, 1), (20, 20), (0, 2)]], (OUTSIDE,)),    # one column: no sample has a right tap
]


# ------------------------------------------------------------------------------------------------------------------
# per-sample prediction
# ------------------------------------------------------------------------------------------------------------------
def warp_src_xy(inv):
    """source coordinates of the S x S output pixels: the f32 operations of oracle_stages' warp_src_xy (tests/test_reference_fixtures.py),
    in the order of imageproc's Projection * (x, y)"""
    inv = np.asarray(inv, dtype=np.float32).reshape(9)
    xs, ys = np.meshgrid(np.arange(S, dtype=np.float32), np.arange(S, dtype=np.float32))
    with np.errstate(all="ignore"):
        den = inv[6] * xs + inv[7] * ys + inv[8]
        px = (inv[0] * xs + inv[1] * ys + inv[2]) / den
        py = (inv[3] * xs + inv[4] * ys + inv[5]) / den
    assert px.dtype == np.float32 and py.dtype == np.float32
    return px, py


def sample_modes(oracle, quads, w, h, bpp, row_stride):
    """-> int64 [3]: samples of all quads' patches per case (OUTSIDE, TAIL, WIDE) on a frame of this layout.  A quad whose projection has no
    solution is sampled nowhere (quirk Q4) and counts nothing."""
    counts = np.zeros(3, dtype=np.int64)
    to = np.array([0, 0, S, 0, S, S, 0, S], np.float32)
    fb = frame_bytes(w, h, bpp, row_stride)
    for q in np.asarray(quads).reshape(-1, 8):
        ok, _, inv = oracle.from_control_points(q.astype(np.float32), to)
        if not ok:
            continue
        px, py = warp_src_xy(inv)
        with np.errstate(all="ignore"):
            left, top = np.floor(px), np.floor(py)
            # (as the sampler writes it: a NaN coordinate fails none of the four tests and reads pixel (0, 0))
            inside = ~((left < 0) | (left + np.float32(1) >= np.float32(w)) | (top < 0) | (top + np.float32(1) >= np.float32(h)))
        l = np.where(inside, np.nan_to_num(left, nan=0.0), 0).astype(np.int64)
        b = np.where(inside, np.nan_to_num(top, nan=0.0) + 1, 0).astype(np.int64)
        tail = inside & (b * row_stride + l * bpp > fb - 12)
        counts += [int((~inside).sum()), int(tail.sum()), int((inside & ~tail).sum())]
    return counts


# ------------------------------------------------------------------------------------------------------------------
# group b: frames whose candidates the contour stage finds itself (the injection hook reaches frame 0 only)
# ------------------------------------------------------------------------------------------------------------------
def _inside_convex(poly, xs, ys):
    m = np.ones(xs.shape, dtype=bool)
    for i in range(4):
        (x0, y0), (x1, y1) = poly[i], poly[(i + 1) % 4]
        m &= (x1 - x0) * (ys - y0) - (y1 - y0) * (xs - x0) >= 0
    return m


def quad_frames(seed, n, h, w, fmt):
    """n textured frames [n, h, w, c]: mid-grey noise, and per frame a light noisy quadrilateral (two where the frame has room) inside a
    dark noisy border -- the inner outline is a border the contour stage turns into a candidate, and every tap of its patch lands on noise"""
    r = np.random.default_rng(seed)
    c = BPP[fmt]
    out = r.integers(90, 171, (n, h, w, c), dtype=np.uint8)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    m = min(w, h)
    spots = [(0.5, 0.5, 0.36)] if w < 90 else [(0.3, 0.45, 0.27), (0.73, 0.55, 0.22)]
    for f in range(n):
        for fx, fy, fr in spots:
            cx, cy = fx * w + r.uniform(-2, 2), fy * h + r.uniform(-2, 2)
            rad = fr * m * r.uniform(0.9, 1.05)
            a0 = r.uniform(0, 2 * np.pi)
            ang = a0 + np.pi / 2 * np.arange(4) + r.uniform(-0.12, 0.12, 4)
            for radius, lo, hi in ((rad + 4.5, 0, 41), (rad, 190, 256)):
                poly = [(cx + radius * np.cos(a), cy + radius * np.sin(a)) for a in ang]
                mask = _inside_convex(poly, xs, ys)
                out[f][mask] = r.integers(lo, hi, (int(mask.sum()), c), dtype=np.uint8)
    if c == 4:
        out[..., 3] = r.integers(0, 256, (n, h, w), dtype=np.uint8)     # alpha is ignored: anything
    return out


FOUND_CASES = [   # (frames, w, h, lead, row pad, frame gap): the gap is odd, so the frames' misalignments differ
    (5, 96, 80, 1, 5, 13),      # k_decode<256, 256>
    (70, 48, 40, 3, 3, 13),     # more than 64 frames: k_decode<256, 64>
]
FOUND_FORMATS = ("RGB8", "BGRA8")


# ------------------------------------------------------------------------------------------------------------------
# group a / d: layouts of one frame with quad_set's quads
# ------------------------------------------------------------------------------------------------------------------
A_SIZE = (61, 47)
A_FORMATS = ("L8", "RGB8", "RGBA8", "BGRA8")
A_LEADS = (0, 1, 2, 3)
A_PADS = (0, 1, 2, 3, 13)

# (format, w, h, row_stride): strides at the edge between the two offset widths, and a frame beyond 4 GiB
D_STRIDE_CASES = [(fmt, 64, 24, rs) for fmt in ("L8", "RGB8") for rs in ((1 << 24) - 4, 1 << 24, (1 << 24) + 1, (1 << 24) + 3)]
D_HEIGHT_CASES = [("L8", 64, 512, 1 << 23), ("L8", 64, 513, 1 << 23)]
