// The argument checks of boards (aruco3_amd/csrc/a3_board3d_check.h): every refusal of a3_set_board3d and of a3_set_board with its message,
// the first failing test deciding, every boundary that passes (sides, angles and planarity at exactly the tolerance, a marker in a plane
// that is not axis-aligned, a planar square in each of its four rotations), and the settings that are refused while a 3-D board is set.  Exits 0 and prints "ok: <n> checks" when every answer
// is the expected one.  tests/test_board3d_checks.py compiles this with the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../aruco3_amd/csrc/a3_board3d_check.h"

namespace {

int g_checks = 0, g_failed = 0;

void same(const char* name, const char* got, const char* want) {
    g_checks++;
    if ((got == nullptr) != (want == nullptr) || (got && std::strcmp(got, want) != 0)) {
        std::printf("FAILED %s: got \"%s\", expected \"%s\"\n", name, got ? got : "OK", want ? want : "OK");
        g_failed++;
    }
}

struct P { float x, y, z; };
const char* marker(P a, P b, P c, P d) {
    const std::vector<float> v{a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z, d.x, d.y, d.z};   // (exactly twelve: a read past them is the sanitizer's to find)
    return a3::check_board3d_marker(v.data());
}

struct Q { float x, y; };
const char* planar(Q a, Q b, Q c, Q d) {
    const std::vector<float> v{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};   // (exactly eight)
    return a3::check_board_marker(v.data());
}

constexpr const char* kFinite2 = "a3_set_board: a corner is not finite";
constexpr const char* kSize2 = "a3_set_board: a marker has no size";
constexpr const char* kSides2 = "a3_set_board: a marker's sides differ (its corners must form a square)";
constexpr const char* kAngles2 = "a3_set_board: a marker's corners are not at right angles (they must form a square)";
constexpr const char* kWinding2 = "a3_set_board: a marker is wound the wrong way (corner order top-left, top-right, bottom-right, bottom-left with y up)";
constexpr const char* kMany2 = "a3_set_board: more than A3_BOARD_MAX_MARKERS markers";
constexpr const char* kNull2 = "a3_set_board: null ids or corners";
constexpr const char* kFinite = "a3_set_board3d: a corner is not finite";
constexpr const char* kSize = "a3_set_board3d: a marker has no size";
constexpr const char* kSides = "a3_set_board3d: a marker's sides differ (its corners must form a square)";
constexpr const char* kAngles = "a3_set_board3d: a marker's corners are not at right angles (they must form a square)";
constexpr const char* kPlane = "a3_set_board3d: a marker's corners do not lie in one plane (they must form a square)";
constexpr const char* kBusy = "a3_set_board3d: a submitted batch has not been collected";
constexpr const char* kMany = "a3_set_board3d: more than A3_BOARD_MAX_MARKERS markers";
constexpr const char* kNull = "a3_set_board3d: null ids or corners";
constexpr const char* kCharuco = "a3_set_charuco: the board is a 3-D board (a3_set_board3d); ChArUco needs a planar one (a3_set_board)";
constexpr const char* kRecovery = "a3_set_board_recovery: the board is a 3-D board (a3_set_board3d); recovery needs a planar one (a3_set_board)";
constexpr const char* kRecoverMarkers = "a3_recover_markers: the board is a 3-D board (a3_set_board3d); recovery needs a planar one (a3_set_board)";

}  // namespace

int main() {
    static_assert(A3_BOARD_MAX_MARKERS == 1024, "the header's limit");
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // ---- one marker: accepted ----
    same("square_xy", marker({0, 0, 0}, {10, 0, 0}, {10, -10, 0}, {0, -10, 0}), nullptr);
    same("square_xy_seen_from_below", marker({0, 0, 0}, {0, -10, 0}, {10, -10, 0}, {10, 0, 0}), nullptr);   // (the order defines the printed side)
    same("square_yz", marker({5, 0, 10}, {5, 10, 10}, {5, 10, 0}, {5, 0, 0}), nullptr);
    {   // a square of side 37.5 in a plane that is no coordinate plane: e_x, e_y two orthonormal vectors with irrational components
        const double ex[3] = {2.0 / 7, 3.0 / 7, 6.0 / 7}, ey[3] = {3.0 / 7, -6.0 / 7, 2.0 / 7}, c[3] = {-12.5, 40.25, 7.0}, h = 18.75;
        P q[4];
        const int sx[4] = {-1, 1, 1, -1}, sy[4] = {1, 1, -1, -1};
        for (int k = 0; k < 4; k++)
            q[k] = {(float)(c[0] + h * (sx[k] * ex[0] + sy[k] * ey[0])), (float)(c[1] + h * (sx[k] * ex[1] + sy[k] * ey[1])),
                    (float)(c[2] + h * (sx[k] * ex[2] + sy[k] * ey[2]))};
        same("square_oblique_plane", marker(q[0], q[1], q[2], q[3]), nullptr);
    }
    same("tiny", marker({0, 0, 0}, {1e-20f, 0, 0}, {1e-20f, -1e-20f, 0}, {0, -1e-20f, 0}), nullptr);
    // ... at exactly the tolerance (s = 1000: 1e-3 s = 1 and 1e-3 s^2 = 1000 exactly, in double)
    same("sides_at_tol", marker({0, 0, 0}, {1000, 0, 0}, {1000, -1001, 0}, {0, -1001, 0}), nullptr);
    same("sides_at_tol_short", marker({0, 0, 0}, {1000, 0, 0}, {1000, -999, 0}, {0, -999, 0}), nullptr);
    same("angles_at_tol", marker({0, 0, 0}, {1000, 0, 0}, {1001, -1000, 0}, {1, -1000, 0}), nullptr);
    same("plane_at_tol", marker({0, 0, 0}, {1000, 0, 0}, {1000, -1000, 1}, {0, -1000, 0}), nullptr);
    // ---- one marker: refused, each from its first failing test ----
    same("nan_first", marker({nan, 0, 0}, {10, 0, 0}, {10, -10, 0}, {0, -10, 0}), kFinite);
    same("inf_last", marker({0, 0, 0}, {10, 0, 0}, {10, -10, 0}, {0, -10, inf}), kFinite);
    same("nan_and_no_size", marker({nan, nan, nan}, {nan, nan, nan}, {nan, nan, nan}, {nan, nan, nan}), kFinite);
    same("no_size", marker({3, 4, 5}, {3, 4, 5}, {3, 4, 5}, {3, 4, 5}), kSize);
    same("no_size_first_side", marker({0, 0, 0}, {0, 0, 0}, {10, -10, 0}, {0, -10, 0}), kSize);   // (before the sides are compared)
    same("sides_past_tol", marker({0, 0, 0}, {1000, 0, 0}, {1000, -1001.5f, 0}, {0, -1001.5f, 0}), kSides);
    same("sides_past_tol_short", marker({0, 0, 0}, {1000, 0, 0}, {1000, -998.5f, 0}, {0, -998.5f, 0}), kSides);
    same("rectangle", marker({0, 0, 0}, {10, 0, 0}, {10, -12, 0}, {0, -12, 0}), kSides);
    same("angles_past_tol", marker({0, 0, 0}, {1000, 0, 0}, {1002, -1000, 0}, {2, -1000, 0}), kAngles);
    same("rhombus", marker({0, 0, 0}, {10, 0, 0}, {16, -8, 0}, {6, -8, 0}), kAngles);
    same("rhombus_before_later_side", marker({0, 0, 0}, {10, 0, 0}, {16, -8, 0}, {6, -9, 0}), kAngles);   // (corner 0's angle comes before side 2)
    same("side_before_its_angle", marker({0, 0, 0}, {10, 0, 0}, {10, -12, 0}, {3, -9, 0}), kSides);       // (side 1 comes before corner 1's angle)
    same("plane_past_tol", marker({0, 0, 0}, {1000, 0, 0}, {1000, -1000, 2}, {0, -1000, 0}), kPlane);
    same("folded", marker({0, 0, 0}, {10, 0, 0}, {10, -10, 0.2f}, {0, -10, 0}), kPlane);
    // ---- the call ----
    const uint32_t id = 0;
    const float xyz[12] = {0, 0, 0, 10, 0, 0, 10, -10, 0, 0, -10, 0};
    same("call_ok", a3::check_board3d_call(false, &id, xyz, 1), nullptr);
    same("call_clear", a3::check_board3d_call(false, nullptr, nullptr, 0), nullptr);
    same("call_most", a3::check_board3d_call(false, &id, xyz, A3_BOARD_MAX_MARKERS), nullptr);
    same("call_busy", a3::check_board3d_call(true, &id, xyz, 1), kBusy);
    same("call_busy_first", a3::check_board3d_call(true, nullptr, nullptr, A3_BOARD_MAX_MARKERS + 1), kBusy);
    same("call_busy_clear", a3::check_board3d_call(true, nullptr, nullptr, 0), kBusy);
    same("call_many", a3::check_board3d_call(false, &id, xyz, A3_BOARD_MAX_MARKERS + 1), kMany);
    same("call_many_before_null", a3::check_board3d_call(false, nullptr, nullptr, A3_BOARD_MAX_MARKERS + 1), kMany);
    same("call_null_ids", a3::check_board3d_call(false, nullptr, xyz, 1), kNull);
    same("call_null_corners", a3::check_board3d_call(false, &id, nullptr, 1), kNull);
    // ---- one planar marker: accepted, in each of the four rotations of the square (the corner order turns with it) ----
    same("planar_square", planar({0, 0}, {10, 0}, {10, -10}, {0, -10}), nullptr);
    same("planar_square_quarter_turn", planar({0, 0}, {0, 10}, {10, 10}, {10, 0}), nullptr);
    same("planar_square_half_turn", planar({0, 0}, {-10, 0}, {-10, 10}, {0, 10}), nullptr);
    same("planar_square_three_quarter_turn", planar({0, 0}, {0, -10}, {-10, -10}, {-10, 0}), nullptr);
    same("planar_square_oblique", planar({3, 4}, {6, 8}, {10, 5}, {7, 1}), nullptr);   // (sides (3, 4), (4, -3): exact)
    same("planar_tiny", planar({0, 0}, {1e-20f, 0}, {1e-20f, -1e-20f}, {0, -1e-20f}), nullptr);
    // ... at exactly the tolerance (s = 1000: 1e-3 s = 1 and 1e-3 s^2 = 1000 exactly, in double), and just outside it
    same("planar_sides_at_tol", planar({0, 0}, {1000, 0}, {1000, -1001}, {0, -1001}), nullptr);
    same("planar_sides_at_tol_short", planar({0, 0}, {1000, 0}, {1000, -999}, {0, -999}), nullptr);
    same("planar_angles_at_tol", planar({0, 0}, {1000, 0}, {1001, -1000}, {1, -1000}), nullptr);
    same("planar_sides_past_tol", planar({0, 0}, {1000, 0}, {1000, -1001.5f}, {0, -1001.5f}), kSides2);
    same("planar_sides_past_tol_short", planar({0, 0}, {1000, 0}, {1000, -998.5f}, {0, -998.5f}), kSides2);
    same("planar_angles_past_tol", planar({0, 0}, {1000, 0}, {1002, -1000}, {2, -1000}), kAngles2);
    // ---- one planar marker: refused, each from its first failing test ----
    same("planar_nan_first", planar({nan, 0}, {10, 0}, {10, -10}, {0, -10}), kFinite2);
    same("planar_inf_last", planar({0, 0}, {10, 0}, {10, -10}, {0, inf}), kFinite2);
    same("planar_no_size", planar({3, 4}, {3, 4}, {3, 4}, {3, 4}), kSize2);
    same("planar_no_size_first_side", planar({0, 0}, {0, 0}, {10, -10}, {0, -10}), kSize2);   // (before the sides are compared)
    same("planar_rectangle", planar({0, 0}, {10, 0}, {10, -12}, {0, -12}), kSides2);
    same("planar_rhombus", planar({0, 0}, {10, 0}, {16, -8}, {6, -8}), kAngles2);
    same("planar_side_before_its_angle", planar({0, 0}, {10, 0}, {10, -12}, {3, -9}), kSides2);   // (side 1 comes before corner 1's angle)
    same("planar_wound_the_other_way", planar({0, 0}, {0, -10}, {10, -10}, {10, 0}), kWinding2);
    same("planar_square_before_winding", planar({0, 0}, {0, -12}, {10, -12}, {10, 0}), kSides2);   // (the winding is the last test)
    // ---- a3_set_board's call ----
    const float xy[8] = {0, 0, 10, 0, 10, -10, 0, -10};
    same("planar_call_ok", a3::check_board_call(&id, xy, 1), nullptr);
    same("planar_call_clear", a3::check_board_call(nullptr, nullptr, 0), nullptr);
    same("planar_call_most", a3::check_board_call(&id, xy, A3_BOARD_MAX_MARKERS), nullptr);
    same("planar_call_many", a3::check_board_call(&id, xy, A3_BOARD_MAX_MARKERS + 1), kMany2);
    same("planar_call_many_before_null", a3::check_board_call(nullptr, nullptr, A3_BOARD_MAX_MARKERS + 1), kMany2);
    same("planar_call_null_ids", a3::check_board_call(nullptr, xy, 1), kNull2);
    same("planar_call_null_corners", a3::check_board_call(&id, nullptr, 1), kNull2);
    // ---- the settings that need a plane ----
    same("charuco_planar", a3::check_charuco_board_kind(false, 24), nullptr);
    same("charuco_3d", a3::check_charuco_board_kind(true, 24), kCharuco);
    same("charuco_3d_clear", a3::check_charuco_board_kind(true, 0), nullptr);
    same("recovery_planar", a3::check_recovery_board_kind(false, 1), nullptr);
    same("recovery_3d", a3::check_recovery_board_kind(true, 1), kRecovery);
    same("recovery_3d_off", a3::check_recovery_board_kind(true, 0), nullptr);
    same("recover_markers_planar", a3::check_recover_markers_board_kind(false), nullptr);
    same("recover_markers_3d", a3::check_recover_markers_board_kind(true), kRecoverMarkers);
    if (g_failed) { std::printf("%d of %d checks FAILED\n", g_failed, g_checks); return 1; }
    std::printf("ok: %d checks\n", g_checks);
    return 0;
}
