"""Three 640 x 480 frames of a 3 x 2 GridBoard for the board-aided marker recovery, rendered on the host (aruco3_amd.synth's renderer,
black cells printed on a flat background) from cell matrices damaged the way tests/damage_util.py damages them (flipped interior
cells; a lit border cell over a black rim, so that the contour stage still finds the square), and what the contract makes of them
from the CPU oracle's detection.  Frame 0 is intact; frame 1 has one marker whose
code lies tau cells from its own (the decoder refuses it, the derived default takes it) and one with a notched border (no code at
all: only a recovery that compares no bits takes it); frame 2 shows a single marker.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from aruco3_amd import synth
from aruco3_amd.board import CharucoBoard, GridBoard
from tests import damage_util as du
from tests import recover_cases, recover_oracle

W, H = du.W, du.H
DICT = recover_cases.DICT
NUM_BITS = DICT.num_bits
N = du.side_cells(NUM_BITS) + 2
CELL = du.CELL["b"][N]
SIDE = N * CELL                 # 147 px
GAP = 53                        # between markers: a 200 px pitch
X0, Y0 = 46, 60                 # the top-left corner of marker (0, 0)
FIRST_ID = 10
DAMAGED_SLOT, NOTCHED_SLOT = 2, 4
FLIPPED = ((0, 0), (2, 3), (4, 1))   # tau interior cells


def board():
    """one board unit = one pixel; the board's origin is the top-left corner of marker (0, 0), y up"""
    return GridBoard(3, 2, float(SIDE), float(GAP), first_id=FIRST_ID)


CHARUCO_CELL = 16               # a smaller drawing: a 4 x 3 chessboard of 150 px squares fills the frame
CHARUCO_ORIGIN = (20, 15)


def charuco_board():
    """a 4 x 3 chessboard of 150-unit squares, six markers of 112 units (only the markers are painted)"""
    return CharucoBoard(4, 3, 150.0, float(N * CHARUCO_CELL), first_id=FIRST_ID)


def cells_of(id_: int):
    return du._framed(du.matrix_of(int(DICT.code_list[id_]), NUM_BITS))


BACKGROUND = 200.0
SPEC = synth.SynthSpec(W, H, paper=True, supersample=3)


def paint(grey, x0: int, y0: int, cells, cell: int = CELL):
    """one upright marker into the float frame `grey`; a lit cell of the top border keeps a two-pixel black rim"""
    side = N * cell
    assert x0 >= cell and y0 >= cell and x0 + side + cell <= W and y0 + side + cell <= H
    quad = np.array([[x0, y0], [x0 + side, y0], [x0 + side, y0 + side], [x0, y0 + side]], np.float64)
    synth._draw_marker(grey, cells, quad, SPEC)
    if cells[0].any():
        grey[y0: y0 + 2, x0: x0 + side] = float(SPEC.black)


def place(b, origin=(X0, Y0)):
    """the top-left pixel of every board marker"""
    c = np.asarray(b.corners, np.float64)[:, 0, :]
    return [(int(round(origin[0] + x)), int(round(origin[1] - y))) for x, y in c]


def frames(b=None, origin=(X0, Y0), cell: int = CELL):
    """-> L8 frames [3, H, W]"""
    b = b or board()
    spots = place(b, origin)
    out = np.full((3, H, W), BACKGROUND, np.float32)
    for f, slots in enumerate((range(len(b)), range(len(b)), (0,))):
        for s in slots:
            cells = cells_of(int(b.ids[s]))
            if f == 1 and s == DAMAGED_SLOT:
                for r, c in FLIPPED:
                    cells[1 + r, 1 + c] ^= 1
            if f == 1 and s == NOTCHED_SLOT:
                cells[0, 3] = 1
            paint(out[f], *spots[s], cells, cell)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def charuco_frames():
    return frames(charuco_board(), CHARUCO_ORIGIN, CHARUCO_CELL)


def oracle_config(oracle):
    return oracle.Config.default()


def detector_config():
    from aruco3_amd.aruco import DetectorConfig

    return DetectorConfig()


def expected(oracle, imgs, b, min_markers: int, max_distance_px: float, max_hamming: int):
    """the contract's merged list of a batch from the CPU oracle's detection of its frames -> (marker tuples as tests.util.marker_tuples
    makes them, per-frame counts, recovered per frame)"""
    merged, per, rec = [], [], []
    for f, img in enumerate(imgs):
        ref = oracle.detect(img, DICT.code_list, NUM_BITS, DICT._tau, config=oracle_config(oracle), keep_debug=False)
        det = ref["markers"]
        taken = {m["candidate_index"] for m in det}
        rejected = np.array([c for c in range(len(ref["candidates"])) if c not in taken], np.int64)
        has = (ref["homography_ok"].astype(bool) & (ref["decode_ok"] != 0)).astype(np.uint8)
        got = recover_oracle.recover_markers(b, DICT.code_list, [m["id"] for m in det], [m["corners"] for m in det], ref["candidates"][rejected],
                                             ref["codes"][rejected], has[rejected], min_markers, max_distance_px, max_hamming, frame=f)
        for m in det:
            merged.append((f, m["id"], m["code"], tuple(v for xy in m["corners"] for v in xy), m["hamming_distance"], m["rotation"], m["candidate_index"]))
        for m in got:
            merged.append((f, int(m["id"]), int(m["code"]), tuple(int(v) for v in m["corners"]), int(m["hamming_distance"]), int(m["rotation"]),
                           int(rejected[int(m["candidate_index"])])))
        per.append(len(det) + len(got))
        rec.append(len(got))
    return merged, per, rec
