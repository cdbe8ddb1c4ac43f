"""Host-side mirror of src/aruco.rs: `Detector`, `DetectorConfig`, `Detection`, `Marker`.

Same names, same fields, same argument meaning as the reference; the body of
`Detector.detect` is one call into the HIP library (batch of 1).  `detect_batch` is the
natural extension the GPU wants: many independent frames per call, on device memory when
the caller already has them there (torch tensors are accepted for that).
"""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from . import _lib
from .dictionaries import ARDictionary


@dataclass
class DetectorConfig:
    """src/aruco.rs:23-43"""
    threshold_window: int = 7
    contour_simplification_epsilon: float = 0.05
    min_side_length_factor: float = 0.2
    min_corner_separation_factor: float = 0.1
    homography_sample_size: int = 49
    filter_high_bit_errors: bool = True

    @classmethod
    def default(cls) -> "DetectorConfig":
        return cls()

    def _c(self) -> _lib.Config:
        return _lib.Config(self.threshold_window, self.contour_simplification_epsilon, self.min_side_length_factor,
                           self.min_corner_separation_factor, self.homography_sample_size, int(self.filter_high_bit_errors))


@dataclass
class CornerRefinement:
    """Sub-pixel corner refinement (a3_refine_config; not in the reference -- include/aruco3_hip.h states the algorithm).
    Passing one to `Detector(refinement=...)` fills `Marker.corners_refined` and makes the pose calls solve from those corners."""
    win_half: int = 5
    relative_win: float = 0.4
    max_iterations: int = 30
    min_shift: float = 0.01
    method: str = "subpix"   # "subpix": a cornerSubPix window around each corner; "edges": lines fitted to the sides, intersected

    @classmethod
    def edges(cls, win_half: int = 10, relative_win: float = 0.4, max_iterations: int = 30, min_shift: float = 0.01) -> "CornerRefinement":
        """Edge-fit refinement (A3_REFINE_EDGES): each corner is where the lines fitted to its two sides cross.  `win_half` is the range
        each side's edge is searched in; the default 10 is what corners mapped up from a reduced plane (`Reduction`) want.  The fit
        assumes straight sides: on frames of an uncorrected lens use "subpix", or a `Rectification`."""
        return cls(win_half, relative_win, max_iterations, min_shift, "edges")

    def _c(self) -> _lib.RefineConfig:
        methods = {"subpix": _lib.REFINE_SUBPIX, "edges": _lib.REFINE_EDGES}
        if self.method not in methods:
            raise ValueError(f"CornerRefinement.method must be one of {sorted(methods)}, not {self.method!r}")
        return _lib.RefineConfig(methods[self.method], self.win_half, self.relative_win, self.max_iterations, self.min_shift)


@dataclass
class Rectification:
    """Frame rectification inside the detect calls (a3_set_rectification; not in the reference).  The arguments mean what they mean in
    `rectify_frames`: `intrinsics` is the camera the frames come from (with its `distortion`), `new_intrinsics` the rectified view and its
    size (default: the camera without its lens), `rotation` 3 x 3 camera -> view, `fill` the grey level of a pixel that sees nothing.
    Passing one to `Detector(rectification=...)` makes every detect call take frames of `intrinsics`' size and return, to the bit, what
    `rectify_frames` followed by the same call would: corners are pixels of the view, and pose calls take the view's plain intrinsics."""
    intrinsics: object
    new_intrinsics: object = None
    rotation: object = None
    fill: int = 0

    def _c(self) -> _lib.RectifyRec:
        from .rectify import rectify_rec

        return rectify_rec(self.intrinsics, self.new_intrinsics, self.rotation, self.fill)

    @property
    def view_size(self) -> Tuple[int, int]:
        """(width, height) of the rectified view"""
        v = self.new_intrinsics if self.new_intrinsics is not None else self.intrinsics
        return int(v.image_width), int(v.image_height)


def _apply_rectification(ctx: _lib.Context, rectification: Optional[Rectification]) -> None:
    """hands a rectification setting to a context that has no batch in flight (the setter is refused otherwise): only on a change"""
    key = None if rectification is None else bytes(rectification._c())
    if getattr(ctx, "_rectification_key", None) != key:
        ctx.set_rectification(None if rectification is None else rectification._c())
        ctx._rectification_key = key


@dataclass
class Reduction:
    """Detection on reduced frames (a3_set_reduction; not in the reference): `Detector(reduction=Reduction(2))` thresholds, traces and
    decodes the frames box-filtered to 1 / `factor` (2, 3 or 4) of their size -- the plane `reduce_frames` returns -- maps the integer
    corners back up (f x + f // 2) and refines them, interpolates ChArUco corners and solves poses on the full-size frames.  For markers
    that are large in the frame; the refinement window has to cover a start that is up to about factor + 1 px off."""
    factor: int

    def _c(self) -> _lib.ReductionRec:
        from .reduce import reduction_rec

        return reduction_rec(self.factor)


def _apply_reduction(ctx: _lib.Context, reduction: Optional[Reduction]) -> None:
    """hands a reduction setting to a context that has no batch in flight (the setter is refused otherwise): only on a change"""
    key = None if reduction is None else bytes(reduction._c())
    if getattr(ctx, "_reduction_key", None) != key:
        ctx.set_reduction(None if reduction is None else reduction._c())
        ctx._reduction_key = key


def _windows_key(threshold_windows) -> tuple:
    """`threshold_windows` as the tuple of radii a3_set_threshold_windows takes (None or empty: off)"""
    return () if threshold_windows is None else tuple(int(v) for v in threshold_windows)


def _apply_threshold_windows(ctx: _lib.Context, threshold_windows) -> None:
    """hands a threshold-window set to a context that has no batch in flight (the setter is refused otherwise): only on a change"""
    key = _windows_key(threshold_windows)
    if getattr(ctx, "_windows_key", ()) != key:
        ctx.set_threshold_windows(key)
        ctx._windows_key = key


def _apply_polarity(ctx: _lib.Context, inverted_markers: bool) -> None:
    """hands the marker polarity (a3_set_marker_polarity) to a context: only on a change"""
    mode = _lib.POLARITY_BOTH if inverted_markers else _lib.POLARITY_DARK
    if getattr(ctx, "_polarity", _lib.POLARITY_DARK) != mode:
        ctx.set_marker_polarity(mode)
        ctx._polarity = mode


def _one_view(reduction, rectification) -> None:
    if reduction is not None and rectification is not None:
        raise ValueError("a detector takes a reduction or a rectification, not both (a3_set_reduction refuses the pair)")


@dataclass
class Marker:
    """src/aruco.rs:8-13, plus whether the marker was recovered through the board (an extension), the refined corners when the detector refines them and the undistorted corners (with their residuals in
    pixels, +inf: not undistorted) when a pose call's intrinsics carry a lens distortion (extensions; None otherwise)"""
    id: int
    code: int
    corners: List[Tuple[int, int]]
    hamming_distance: int
    corners_refined: Optional[List[Tuple[float, float]]] = None
    corners_undistorted: Optional[List[Tuple[float, float]]] = None
    undistort_residual_px: Optional[List[float]] = None
    recovered: bool = False   # with Detector(recovery=...): the decoder rejected this quad, the board placed it (hamming_distance 255: bits not compared)
    inverted: bool = False    # with Detector(inverted_markers=True): the marker is bright on dark and was read complemented (a3_get_marker_flags)


@dataclass
class Detection:
    """src/aruco.rs:15-21.  grey / candidates / homographies are filled on request only (populate=True):
    copying 2 MB per 1080p frame back to the host would dominate the call."""
    grey: Optional[np.ndarray] = None
    candidates: List[List[Tuple[int, int]]] = field(default_factory=list)
    homographies: List[np.ndarray] = field(default_factory=list)
    markers: List[Marker] = field(default_factory=list)
    # with a CharucoBoard as the detector's board (an extension): the chessboard corners found, ids (n,) uint32 ascending and
    # raw image pixels (n, 2) float32 -- refined, or interpolated with CharucoConfig.refine = 0; None otherwise
    charuco_ids: Optional[np.ndarray] = None
    charuco_corners: Optional[np.ndarray] = None


PACKED_422 = {"yuyv": _lib.FMT_YUYV8, "uyvy": _lib.FMT_UYVY8}   # 2 bytes per pixel; the luma byte is the grey level as it stands
PLANAR_LUMA_FIRST = ("nv12", "nv21", "i420", "yv12")               # H rows of luma, then H / 2 rows of chroma in some order


def _as_frames(image, pixel_format: Optional[str] = None):
    """The one place that understands frame layouts.  -> (pointer, memory kind, fmt, w, h, row_stride, frame_stride, n, keepalive)

    pixel_format None: the format follows from the channel count -- (N,H,W,C), (H,W,C) or (H,W) uint8 with C 1 (L8), 3 (RGB8) or 4
    (RGBA8); two channels are refused (YUYV or UYVY: the byte order is the caller's to say).
    "bgra": 4 channels in webcam byte order B,G,R,A.
    "yuyv" / "uyvy": packed 4:2:2, (N,H,W,2) or (H,W,2), W even; the luma byte of every pixel is its grey level, chroma is never read
    into a result.
    "nv12", "nv21", "i420", "yv12": the luma-first planar layouts, (N,3H/2,W) or (3H/2,W) -- the buffer as the decoder wrote it.  The
    luma plane is read in place (FMT_L8, height H, row stride W, frame stride 3H/2 * W); the chroma rows are skipped by the strides.
    numpy arrays and torch tensors, on the host or the device; nothing is copied beyond making the buffer contiguous."""
    try:
        import torch
    except ImportError:  # pragma: no cover
        torch = None
    fmt_name = None if pixel_format is None else str(pixel_format).lower()
    if fmt_name is not None and fmt_name != "bgra" and fmt_name not in PACKED_422 and fmt_name not in PLANAR_LUMA_FIRST:
        raise ValueError(f"unknown pixel_format {pixel_format!r}: None, 'bgra', 'yuyv', 'uyvy', 'nv12', 'nv21', 'i420' or 'yv12'")
    is_tensor = torch is not None and isinstance(image, torch.Tensor)
    a = image if is_tensor else np.asarray(image)
    if a.dtype != (torch.uint8 if is_tensor else np.uint8):
        raise TypeError("frames must be uint8")
    nd = a.dim() if is_tensor else a.ndim
    if fmt_name in PLANAR_LUMA_FIRST:
        if nd == 2:
            a = a[None]
        if (a.dim() if is_tensor else a.ndim) != 3:
            raise ValueError(f"pixel_format={fmt_name!r} expects (N,3H/2,W) or (3H/2,W)")
        n, rows, w = (int(v) for v in a.shape)
        if rows % 3 or (rows * 2 // 3) % 2:
            raise ValueError(f"pixel_format={fmt_name!r}: {rows} rows are not 3H/2 for an even H")
        if w % 2:
            raise ValueError(f"pixel_format={fmt_name!r}: 4:2:0 frames have an even width")
        c, h, fmt, row, frame = 1, rows * 2 // 3, _lib.FMT_L8, w, rows * w
    else:
        chans = (2,) if fmt_name in PACKED_422 else (4,) if fmt_name == "bgra" else (1, 3, 4)
        if nd == 2 and 1 in chans:
            a = a[None, :, :, None]
        elif nd == 3:
            a = a[None] if a.shape[-1] in chans else a[..., None]
        if (a.dim() if is_tensor else a.ndim) != 4 or a.shape[-1] not in chans:
            if fmt_name in PACKED_422:
                raise ValueError(f"pixel_format={fmt_name!r} expects (N,H,W,2) or (H,W,2)")
            if fmt_name == "bgra":
                raise ValueError("bgra=True needs 4-channel frames")
            if nd in (3, 4) and a.shape[-1] == 2:
                raise ValueError("expected (N,H,W,C) with C in 1,3,4; 2-channel frames need pixel_format='yuyv' or 'uyvy'")
            raise ValueError("expected (N,H,W,C) with C in 1,3,4")
        n, h, w, c = (int(v) for v in a.shape)
        if c == 2 and w % 2:
            raise ValueError("4:2:2 frames have an even width")
        fmt = PACKED_422[fmt_name] if c == 2 else _lib.FMT_BGRA8 if fmt_name == "bgra" else {1: _lib.FMT_L8, 3: _lib.FMT_RGB8, 4: _lib.FMT_RGBA8}[c]
        row, frame = w * c, h * w * c
    if is_tensor:
        a = a.contiguous()
        return a.data_ptr(), _lib.MEM_DEVICE if a.is_cuda else _lib.MEM_HOST, fmt, w, h, row, frame, n, a
    a = np.ascontiguousarray(a)
    return a.ctypes.data, _lib.MEM_HOST, fmt, w, h, row, frame, n, a


def _pixel_format(pixel_format: Optional[str], bgra: bool) -> Optional[str]:
    """the pixel_format of a call that also has the older `bgra` flag"""
    if bgra and pixel_format not in (None, "bgra"):
        raise ValueError("bgra=True and pixel_format disagree")
    return "bgra" if bgra else pixel_format


class Detector:
    """`Detector { config, dictionary }` (src/aruco.rs:46-49)."""

    def __init__(self, config: DetectorConfig = None, dictionary: ARDictionary = None, device: int = 0,
                 refinement: Optional[CornerRefinement] = None, board=None, charuco_config: Optional[_lib.CharucoConfig] = None,
                 rectification: Optional[Rectification] = None, recovery=None, reduction: Optional[Reduction] = None,
                 threshold_windows=None, inverted_markers: bool = False):
        _one_view(reduction, rectification)
        if recovery is not None and board is None:
            raise ValueError("Detector(recovery=...) needs a board: recovery places rejected quads where the board says its markers are")
        if recovery is not None and _is_board3d(board):
            raise ValueError("Detector(recovery=...) needs a planar board: a homography places the missing markers, and a Board3D has none")
        self.config = config or DetectorConfig()
        self.dictionary = dictionary or ARDictionary.new_from_named_dict("ARUCO")
        self.device = device
        self.refinement = refinement
        self.board = board   # aruco3_amd.board.Board: detect_batch_with_board_pose solves one pose per frame from it
        # with a board.CharucoBoard: every call also returns the chessboard corners (a3_charuco_config; None: the library's defaults)
        self.charuco_config = charuco_config
        # every call sees its frames through this rectification (frames of its camera's size in, pixels of its view out)
        self.rectification = rectification
        # aruco3_amd.board.BoardRecovery: board markers the decoder rejected are recovered on the device (Marker.recovered)
        self.recovery = recovery
        # the front half of every call runs on the frames reduced by this factor; corners, refinement and poses are full-size
        self.reduction = reduction
        # several adaptive-threshold windows (a3_set_threshold_windows; not in the reference): e.g. (3, 7, 15) -- every frame is
        # binarised at each radius and the candidates are merged on the device; one radius overrides config.threshold_window; None: off
        self.threshold_windows = threshold_windows
        # bright-on-dark markers are read beside dark ones (a3_set_marker_polarity, OpenCV's detectInvertedMarker; not in the
        # reference): Marker.inverted says which.  A bright rectangle is then a candidate marker too: see include/aruco3_hip.h
        self.inverted_markers = inverted_markers
        self._ctx = None
        self._ctx_key = None

    def _apply_refinement(self, ctx: _lib.Context) -> bool:
        """hands the detector's refinement setting to the context before a call -> whether it is on"""
        r = self.refinement
        ctx.set_corner_refinement(r._c() if r is not None else None)
        return r is not None

    def _apply_board(self, ctx: _lib.Context) -> bool:
        """hands the detector's board (and, for a CharucoBoard, its chessboard) to the context before a call -> whether one is set"""
        b, cfg = self.board, self.charuco_config
        key = (b, None if cfg is None else bytes(cfg))
        applied = getattr(self, "_board_applied", None)
        if applied is None or applied[0] is not ctx or applied[1] != key:   # (a3_set_board re-uploads the tables: only on a change)
            _set_board(ctx, b, cfg)
            self._board_applied = (ctx, key)
        return b is not None

    def _apply_recovery(self, ctx: _lib.Context) -> bool:
        """hands the detector's recovery setting (and the board it needs) to the context before a call -> whether it is on"""
        return _apply_recovery(ctx, self.recovery, lambda: self._apply_board(ctx))

    def _charuco(self, ctx: _lib.Context) -> bool:
        """a CharucoBoard as the board: hands it to the context (every call then reports its corners) -> whether it is one"""
        if not _is_charuco(self.board):
            return False
        self._apply_board(ctx)
        return True

    def _apply_distortion(self, ctx: _lib.Context, intrinsics) -> bool:
        """hands the lens distortion of a pose call's intrinsics to the context before the call -> whether it is on"""
        d = getattr(intrinsics, "distortion", None) if intrinsics is not None else None
        ctx.set_distortion(d._c() if d is not None else None)
        return d is not None

    def _check_pose_intrinsics(self, intrinsics) -> None:
        """a detector that rectifies its frames returns pixels of an ideal pinhole view: a lens on the pose call would undistort twice"""
        if self.rectification is not None and getattr(intrinsics, "distortion", None) is not None:
            raise ValueError("the detector rectifies its frames: pass the view's plain intrinsics (no `distortion`) to the pose calls")

    def _context(self) -> _lib.Context:
        _one_view(self.reduction, self.rectification)
        key = (tuple(vars(self.config).items()), id(self.dictionary), self.device)
        if self._ctx is None or self._ctx_key != key:
            d = self.dictionary
            self._ctx = _lib.Context(self.config._c(), d.code_list, d.num_bits, d._tau, self.device)
            self._ctx_key = key
        if self.reduction is None:   # (one of the two at a time: the one that goes is turned off first)
            _apply_reduction(self._ctx, None)
        _apply_rectification(self._ctx, self.rectification)
        _apply_reduction(self._ctx, self.reduction)
        _apply_threshold_windows(self._ctx, self.threshold_windows)
        _apply_polarity(self._ctx, self.inverted_markers)
        return self._ctx

    # src/aruco.rs:52-121
    def detect(self, image, populate: bool = False, pixel_format: Optional[str] = None) -> Detection:
        return self.detect_batch(image, populate=populate, pixel_format=pixel_format)[0]

    def detect_batch(self, images, populate: bool = False, stream: int = None, out_cap: int = 0, bgra: bool = False,
                     pixel_format: Optional[str] = None) -> List[Detection]:
        """`bgra=True` (or pixel_format="bgra"): 4-channel frames are in webcam byte order B,G,R,A (examples/webcam_kamera.rs:38-52
        re-orders them on the CPU before `detect`; here the kernel reads them as they are).
        pixel_format (here and in every call that takes frames): "yuyv" / "uyvy" for packed 4:2:2 frames (N,H,W,2), "nv12" / "nv21" /
        "i420" / "yv12" for planar buffers (N,3H/2,W) -- read in place, the luma byte is the grey level (`_as_frames` states the
        layouts); the result is, to the bit, that of the luma plane as an L8 frame, and `populate=True` returns that plane as `grey`."""
        ctx = self._context()
        ptr, mem, fmt, w, h, rs, fs, n, keep = _as_frames(images, _pixel_format(pixel_format, bgra))
        if stream is not None:
            ctx.set_stream(stream)
        ctx.set_debug_taps(populate)
        refine = self._apply_refinement(ctx)
        charuco = self._charuco(ctx)
        recover = self._apply_recovery(ctx)
        markers, per = ctx.detect_batch(ptr, mem, fmt, w, h, rs, fs, n, out_cap)
        refined = ctx.refined_corners() if refine else None
        rec = ctx.recovered_counts(n) if recover else None
        flags = ctx.marker_flags() if self.inverted_markers else None
        out = []
        pos = 0
        for f in range(n):
            det = Detection()
            for i in range(pos, pos + int(per[f])):
                det.markers.append(_marker(markers[i], refined[i] if refined is not None else None, recovered=_is_tail(rec, f, i - pos, per),
                                           inverted=_inverted_at(flags, i)))
            pos += int(per[f])
            if populate:
                view = (w // self.reduction.factor, h // self.reduction.factor) if self.reduction is not None else (w, h)
                det.grey = ctx.download_grey(f, *(self.rectification.view_size if self.rectification is not None else view))
                det.candidates = [[(int(x), int(y)) for x, y in q] for q in ctx.candidates(f)]
                patches, ok, _, _ = ctx.homographies(f)
                det.homographies = [p if o else np.zeros((1, 1), np.uint8) for p, o in zip(patches, ok)]  # src/aruco.rs:256
            out.append(det)
        if charuco:
            _fill_charuco(out, ctx.charuco_corners())
        return out

    def detect_batch_with_pose(self, images, marker_size_mm: float, intrinsics=None, stream: int = None, out_cap: int = 0,
                               pixel_format: Optional[str] = None):
        """detect + `pose::solve_with_undistorted_points` / `solve_with_intrinsics` of every marker (src/pose.rs:52-81) in one
        device pass, the way examples/webcam_kamera.rs:56-71 chains them.  -> [(Detection, [(MarkerPose, MarkerPose), ...])]"""
        from .pose import MarkerPose

        self._check_pose_intrinsics(intrinsics)
        ctx = self._context()
        ptr, mem, fmt, w, h, rs, fs, n, keep = _as_frames(images, pixel_format)
        if stream is not None:
            ctx.set_stream(stream)
        ctx.set_debug_taps(False)
        refine = self._apply_refinement(ctx)
        dist = self._apply_distortion(ctx, intrinsics)
        charuco = self._charuco(ctx)
        recover = self._apply_recovery(ctx)
        intr = None
        if intrinsics is not None:
            ci = intrinsics
            intr = _lib.Intrinsics(ci.image_width, ci.image_height, ci.focal_x, ci.focal_y, ci.principal_x, ci.principal_y)
        markers, per, poses = ctx.detect_batch_pose(ptr, mem, fmt, w, h, rs, fs, n, marker_size_mm, intr, out_cap)
        refined = ctx.refined_corners() if refine else None
        undist = ctx.undistorted_corners() if dist else None
        rec = ctx.recovered_counts(n) if recover else None
        flags = ctx.marker_flags() if self.inverted_markers else None
        out = []
        pos = 0
        for f in range(n):
            det = Detection()
            pp = []
            for i in range(pos, pos + int(per[f])):
                det.markers.append(_marker(markers[i], refined[i] if refined is not None else None, _undist_at(undist, i), _is_tail(rec, f, i - pos, per),
                                           _inverted_at(flags, i)))
                pp.append(tuple(MarkerPose(float(q[0]), q[1:10].reshape(3, 3).copy(), q[10:13].copy()) for q in poses[i]))
            pos += int(per[f])
            out.append((det, pp))
        if charuco:
            _fill_charuco([d for d, _ in out], ctx.charuco_corners())
        return out

    def detect_batch_with_board_pose(self, images, intrinsics=None, marker_size_mm: float = 1.0, stream: int = None, out_cap: int = 0,
                                     pixel_format: Optional[str] = None):
        """detect + one board pose per frame (the detector's `board`), solved on the device from every board marker of the frame
        (include/aruco3_hip.h states the solve).  -> [(Detection, BoardPose)]; the per-marker poses of the same call are solved too
        (with `marker_size_mm`) and left out here -- detect_batch_with_pose returns them."""
        from .board import BoardPose

        if self.board is None:
            raise ValueError("detect_batch_with_board_pose needs Detector(board=...)")
        self._check_pose_intrinsics(intrinsics)
        ctx = self._context()
        ptr, mem, fmt, w, h, rs, fs, n, keep = _as_frames(images, pixel_format)
        if stream is not None:
            ctx.set_stream(stream)
        ctx.set_debug_taps(False)
        refine = self._apply_refinement(ctx)
        dist = self._apply_distortion(ctx, intrinsics)
        self._apply_board(ctx)
        recover = self._apply_recovery(ctx)
        intr = None
        if intrinsics is not None:
            ci = intrinsics
            intr = _lib.Intrinsics(ci.image_width, ci.image_height, ci.focal_x, ci.focal_y, ci.principal_x, ci.principal_y)
        markers, per, _ = ctx.detect_batch_pose(ptr, mem, fmt, w, h, rs, fs, n, marker_size_mm, intr, out_cap)
        refined = ctx.refined_corners() if refine else None
        undist = ctx.undistorted_corners() if dist else None
        boards = ctx.board_poses()
        dets = _detections(markers, per, refined, undist, ctx.recovered_counts(n) if recover else None,
                           ctx.marker_flags() if self.inverted_markers else None)
        if _is_charuco(self.board):
            _fill_charuco(dets, ctx.charuco_corners())
        return [(d, BoardPose._from(boards[f])) for f, d in enumerate(dets)]

    def detect_batch_with_charuco_pose(self, images, intrinsics=None, marker_size_mm: float = 1.0, stream: int = None, out_cap: int = 0,
                                       pixel_format: Optional[str] = None):
        """detect + the ChArUco corners + one ChArUco pose per frame (the detector's `board`, a CharucoBoard), solved on the device from
        the frame's chessboard corners (include/aruco3_hip.h states the solve).  -> [(Detection, CharucoPose)]"""
        from .board import CharucoPose

        if not _is_charuco(self.board):
            raise ValueError("detect_batch_with_charuco_pose needs Detector(board=CharucoBoard(...))")
        self._check_pose_intrinsics(intrinsics)
        ctx = self._context()
        ptr, mem, fmt, w, h, rs, fs, n, keep = _as_frames(images, pixel_format)
        if stream is not None:
            ctx.set_stream(stream)
        ctx.set_debug_taps(False)
        refine = self._apply_refinement(ctx)
        dist = self._apply_distortion(ctx, intrinsics)
        self._apply_board(ctx)
        recover = self._apply_recovery(ctx)
        intr = None
        if intrinsics is not None:
            ci = intrinsics
            intr = _lib.Intrinsics(ci.image_width, ci.image_height, ci.focal_x, ci.focal_y, ci.principal_x, ci.principal_y)
        markers, per, _ = ctx.detect_batch_pose(ptr, mem, fmt, w, h, rs, fs, n, marker_size_mm, intr, out_cap)
        refined = ctx.refined_corners() if refine else None
        undist = ctx.undistorted_corners() if dist else None
        dets = _detections(markers, per, refined, undist, ctx.recovered_counts(n) if recover else None,
                           ctx.marker_flags() if self.inverted_markers else None)
        _fill_charuco(dets, ctx.charuco_corners())
        poses = ctx.charuco_poses()
        return [(d, CharucoPose._from(poses[f])) for f, d in enumerate(dets)]

    def interpolate_charuco(self, image, ids, corners, pixel_format: Optional[str] = None):
        """stand-alone, one frame (a3_interpolate_charuco): the chessboard corners of the detector's CharucoBoard from caller-given
        markers -- ids (n,) and raw pixel corners (n, 4, 2) -- refined on `image` as a batch refines them.  -> (ids (m,) uint32,
        corners (m, 2) float32)"""
        if not _is_charuco(self.board):
            raise ValueError("interpolate_charuco needs Detector(board=CharucoBoard(...))")
        ctx = self._context()
        ptr, mem, fmt, w, h, rs, fs, n, keep = _as_frames(image, pixel_format)
        if n != 1:
            raise ValueError("interpolate_charuco takes one frame")
        self._apply_board(ctx)
        rec = ctx.interpolate_charuco(ptr, mem, fmt, w, h, rs, ids, corners)
        return rec["id"].copy(), np.stack([rec["x"], rec["y"]], axis=1).astype(np.float32)

    def refine_corners(self, image, corners, cell_px=None, pixel_format: Optional[str] = None) -> np.ndarray:
        """stand-alone, one frame (a3_refine_corners): corners (..., 2) -> refined float32 (n, 2) with the detector's `refinement` (the
        library's defaults without one); cell_px: one marker cell size per corner for the relative window, or None"""
        ctx = self._context()
        ptr, mem, fmt, w, h, rs, fs, n, keep = _as_frames(image, pixel_format)
        if n != 1:
            raise ValueError("refine_corners takes one frame")
        self._apply_refinement(ctx)
        return ctx.refine_corners(ptr, mem, fmt, w, h, rs, corners, cell_px)

    def detect_batch_raw(self, images, stream: int = None, out_cap: int = 0, pixel_format: Optional[str] = None):
        """Batch entry without Python object construction: (structured marker array, per-frame counts)."""
        ctx = self._context()
        ptr, mem, fmt, w, h, rs, fs, n, keep = _as_frames(images, pixel_format)
        if stream is not None:
            ctx.set_stream(stream)
        self._apply_refinement(ctx)   # (the refined corners are not returned here: Context.refined_corners() has them)
        self._apply_recovery(ctx)     # (likewise the recovered counts: Context.recovered_counts())
        return ctx.detect_batch(ptr, mem, fmt, w, h, rs, fs, n, out_cap)


def _is_charuco(board) -> bool:
    from .board import CharucoBoard

    return isinstance(board, CharucoBoard)


def _is_board3d(board) -> bool:
    from .board import Board3D

    return isinstance(board, Board3D)


def _set_board(ctx: _lib.Context, board, charuco_config=None) -> None:
    """a3_set_board (which clears the ChArUco setting), then a3_set_charuco for a CharucoBoard; a3_set_board3d for a Board3D"""
    if _is_board3d(board):
        ctx.set_board3d(board.ids, board.corners)
        return
    ctx.set_board(None if board is None else board.ids, None if board is None else board.corners)
    if _is_charuco(board):
        ctx.set_charuco(board.chessboard_corners, board.adjacent_ids, charuco_config)


def _apply_recovery(ctx: _lib.Context, recovery, apply_board) -> bool:
    """hands a BoardRecovery (or None) to a context that has no batch in flight; apply_board() sets the board it needs first"""
    if recovery is None:
        if getattr(ctx, "_recovery_key", None) is not None:
            ctx.set_board_recovery(None)
            ctx._recovery_key = None
        return False
    apply_board()
    cfg = recovery._c(ctx)
    if getattr(ctx, "_recovery_key", None) != bytes(cfg):
        ctx.set_board_recovery(cfg)
        ctx._recovery_key = bytes(cfg)
    return True


def _is_tail(rec, f: int, k: int, per) -> bool:
    """marker k of frame f's segment is one of the frame's rec[f] recovered markers (they are the segment's tail)"""
    return rec is not None and k >= int(per[f]) - int(rec[f])


def _fill_charuco(dets: List[Detection], recs: np.ndarray) -> None:
    """Detection.charuco_ids / .charuco_corners of each frame from the (frame, id)-ordered records of Context.charuco_corners()"""
    bounds = np.searchsorted(recs["frame"], np.arange(len(dets) + 1))
    for f, d in enumerate(dets):
        r = recs[bounds[f]:bounds[f + 1]]
        d.charuco_ids = r["id"].copy()
        d.charuco_corners = np.stack([r["x"], r["y"]], axis=1).astype(np.float32).reshape(-1, 2)


def _marker(m, refined=None, undist=None, recovered: bool = False, inverted: bool = False) -> Marker:
    c = m["corners"]
    return Marker(int(m["id"]), int(m["code"]), [(int(c[2 * i]), int(c[2 * i + 1])) for i in range(4)], int(m["hamming_distance"]),
                  None if refined is None else [(float(x), float(y)) for x, y in refined],
                  None if undist is None else [(float(x), float(y)) for x, y in undist[0]],
                  None if undist is None else [float(r) for r in undist[1]], recovered, inverted)


def _undist_at(undist, i):
    """marker i's (corners, residuals) of Context.undistorted_corners(), or None"""
    return None if undist is None else (undist[0][i], undist[1][i])


def _inverted_at(flags, i) -> bool:
    """marker i's A3_MARKER_INVERTED bit of Context.marker_flags() (None: the batch ran in mode DARK)"""
    return flags is not None and bool(int(flags[i]) & _lib.MARKER_INVERTED)


def _detections(markers, per, refined=None, undist=None, rec=None, flags=None) -> List[Detection]:
    out, pos = [], 0
    for f in range(len(per)):
        det = Detection()
        for i in range(pos, pos + int(per[f])):
            det.markers.append(_marker(markers[i], refined[i] if refined is not None else None, _undist_at(undist, i), _is_tail(rec, f, i - pos, per),
                                       _inverted_at(flags, i)))
        pos += int(per[f])
        out.append(det)
    return out


class BatchQueue:
    """Several batches in flight -- the Python twin of `BatchQueue` in integration/aruco3_hip.rs (additive API; public entry points of
    include/aruco3_hip.h only).  `depth` contexts of its own are used in rotation, each on a stream of its own: `submit` hands a batch
    over and returns at once, `collect` waits for the OLDEST batch in flight and returns its detections (markers only).

    gates=False (default): a free-running rotation -- with a batch of its own per context the fastest arrangement measured (DESIGN.md
    section 4.4).  gates=True: before each submit context k calls a3_order_after for the contexts k+1 .. depth-1 (bursts): the library
    holds the chain of every member but the last behind its threshold kernel; `last_stepping` says what it did with the batch just
    collected.  Results never depend on any of it.  Frames must stay valid and unmodified until their batch is collected (the queue
    keeps a reference to what it was handed)."""

    def __init__(self, detector: Detector, depth: int = 4, gates: bool = False):
        if not 1 <= depth <= 8:
            raise ValueError("depth must be in 1..8")
        _one_view(detector.reduction, detector.rectification)
        d = detector.dictionary
        self._ctxs = [_lib.Context(detector.config._c(), d.code_list, d.num_bits, d._tau, detector.device) for _ in range(depth)]
        self._refinement = detector.refinement   # (the detector's setting when the queue was made; each batch keeps the one in force at its submit)
        self._board, self._charuco_config = detector.board, detector.charuco_config   # (likewise)
        self._rectification = detector.rectification   # (likewise)
        self._recovery = detector.recovery   # (likewise)
        self._reduction = detector.reduction   # (likewise)
        self._threshold_windows = detector.threshold_windows   # (likewise)
        self._inverted = bool(detector.inverted_markers)   # (likewise)
        self._refine_on = [False] * depth
        self._flags_on = [False] * depth
        self._keep = [None] * depth
        self._pose_batch = [False] * depth
        self._gates = gates
        self._head = self._in_flight = self._submitted = 0
        self.last_stepping = None

    def __len__(self) -> int:
        return self._in_flight

    @property
    def full(self) -> bool:
        return self._in_flight == len(self._ctxs)

    def submit_with_board_pose(self, images, intrinsics=None, marker_size_mm: float = 1.0, out_cap: int = 0,
                               pixel_format: Optional[str] = None) -> None:
        """submit as a pose batch (a3_detect_batch_pose_submit): `collect_with_board_pose` returns what
        Detector.detect_batch_with_board_pose would.  Needs the detector's board (planar or Board3D); no lens distortion is applied."""
        if self._board is None:
            raise ValueError("submit_with_board_pose needs Detector(board=...)")
        intr = None
        if intrinsics is not None:
            ci = intrinsics
            intr = _lib.Intrinsics(ci.image_width, ci.image_height, ci.focal_x, ci.focal_y, ci.principal_x, ci.principal_y)
        self.submit(images, out_cap, pixel_format, _pose=(float(marker_size_mm), intr))

    def collect_with_board_pose(self):
        """the oldest batch in flight, which submit_with_board_pose handed over -> [(Detection, BoardPose)]"""
        from .board import BoardPose

        ctx = self._ctxs[self._head]
        dets = self.collect()
        boards = ctx.board_poses()
        return [(d, BoardPose._from(boards[f])) for f, d in enumerate(dets)]

    def submit(self, images, out_cap: int = 0, pixel_format: Optional[str] = None, _pose=None) -> None:
        if self.full:
            raise RuntimeError("BatchQueue is full: collect() the oldest batch first")
        depth = len(self._ctxs)
        k = self._submitted % depth
        ctx = self._ctxs[k]
        if self._gates:
            for m in range(k + 1, depth):
                ctx.order_after(self._ctxs[m])
        ptr, mem, fmt, w, h, rs, fs, n, keep = _as_frames(images, pixel_format)
        ctx.set_debug_taps(False)
        _apply_rectification(ctx, self._rectification)   # (this context's last batch has been collected: the queue is not full)
        _apply_reduction(ctx, self._reduction)
        _apply_threshold_windows(ctx, self._threshold_windows)
        _apply_polarity(ctx, self._inverted)
        self._flags_on[k] = self._inverted
        ctx.set_corner_refinement(self._refinement._c() if self._refinement is not None else None)
        self._refine_on[k] = self._refinement is not None
        if self._submitted < depth and self._board is not None:   # (each context's first batch: the board stays set on it)
            _set_board(ctx, self._board, self._charuco_config)
        _apply_recovery(ctx, self._recovery, lambda: None)   # (the board is set: Detector refuses a recovery without one)
        if _pose is not None:
            ctx.submit_pose(ptr, mem, fmt, w, h, rs, fs, n, _pose[0], _pose[1], out_cap=out_cap or n * 64)
        else:
            ctx.submit(ptr, mem, fmt, w, h, rs, fs, n, out_cap=out_cap or n * 64)
        self._pose_batch[k] = _pose is not None
        self._keep[k] = keep
        self._submitted += 1
        self._in_flight += 1

    def collect(self) -> List[Detection]:
        if not self._in_flight:
            raise RuntimeError("BatchQueue.collect with nothing in flight")
        k = self._head
        ctx = self._ctxs[k]
        self._head = (self._head + 1) % len(self._ctxs)
        self._in_flight -= 1
        try:
            markers, per = ctx.collect_pose()[:2] if self._pose_batch[k] else ctx.collect()
        finally:
            self._keep[k] = None
        self.last_stepping = ctx.stats()["stepping"]
        dets = _detections(markers, per, ctx.refined_corners() if self._refine_on[k] else None,
                           rec=ctx.recovered_counts(len(per)) if self._recovery is not None else None,
                           flags=ctx.marker_flags() if self._flags_on[k] else None)
        if _is_charuco(self._board):
            _fill_charuco(dets, ctx.charuco_corners())
        return dets

    def close(self) -> None:
        while self._in_flight:
            self.collect()
        for c in self._ctxs:
            c.close()
        self._ctxs = []
