// a3_ippe.h -- the IPPE solver of one square marker (src/pose.rs:64-348; matrices row-major), shared by k_pose (k_decode.hip) and the
// board start of k_board_pose (k_board.hip).  Built with the library's flags (-ffp-contract=off, correctly rounded f32 divide / sqrt),
// so the same points give the same bits in either kernel.
#pragma once

#include "a3_common.h"

namespace a3 {

__device__ inline void find_rotation_to_z(const float v[3], float rot[9]) {  // src/pose.rs:238-267
    for (int i = 0; i < 9; i++) rot[i] = 0.0f;
    const float a = v[0] * v[0], b = v[1] * v[1], c = v[2] * v[2];
    const float nrm = sqrtf(a + b + c);
    const float ax = v[0] / nrm, ay = v[1] / nrm, az = v[2] / nrm;
    if (fabsf(1.0f + az) < 1e-6f) {
        rot[0] = 1.0f; rot[4] = 1.0f; rot[8] = -1.0f;
    } else {
        const float d = 1.0f / (1.0f + az);
        const float ax2 = ax * ax, ay2 = ay * ay, axay = ax * ay;
        rot[0] = -ax2 * d + 1.0f; rot[1] = -axay * d;       rot[2] = -ax;
        rot[3] = -axay * d;       rot[4] = -ay2 * d + 1.0f; rot[5] = -ay;
        rot[6] = ax;              rot[7] = ay;              rot[8] = 1.0f - (ax2 + ay2) * d;
    }
}

__device__ inline void compute_rotations(const float j[4], float tx, float ty, float r1[9], float r2[9]) {  // src/pose.rs:158-235
    const float t[3] = {tx, ty, 1.0f};
    float rz[9], rv[9];
    find_rotation_to_z(t, rz);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) rv[r * 3 + c] = rz[c * 3 + r];
#define RV(r, c) rv[((r) - 1) * 3 + ((c) - 1)]
    const float b00 = RV(1, 1) - tx * RV(3, 1);
    const float b01 = RV(1, 2) - tx * RV(3, 2);
    const float b10 = RV(2, 1) - ty * RV(3, 1);
    const float b11 = RV(2, 2) - ty * RV(3, 2);
    const float inv_det = 1.0f / (b00 * b11 - b01 * b10);
    const float binv00 = inv_det * b11, binv01 = -inv_det * b01, binv10 = -inv_det * b10, binv11 = inv_det * b00;
    const float a00 = binv00 * j[0] + binv01 * j[2];
    const float a01 = binv00 * j[1] + binv01 * j[3];
    const float a10 = binv10 * j[0] + binv11 * j[2];
    const float a11 = binv10 * j[1] + binv11 * j[3];
    const float ata00 = a00 * a00 + a01 * a01;
    const float ata01 = a00 * a10 + a01 * a11;
    const float ata11 = a10 * a10 + a11 * a11;
    const float gamma = sqrtf(0.5f * (ata00 + ata11 + sqrtf((ata00 - ata11) * (ata00 - ata11) + 4.0f * ata01 * ata01)));
    const float rt00 = a00 / gamma, rt01 = a01 / gamma, rt10 = a10 / gamma, rt11 = a11 / gamma;
    const float rt00_2 = rt00 * rt00, rt01_2 = rt01 * rt01, rt10_2 = rt10 * rt10, rt11_2 = rt11 * rt11;
    const float b0 = sqrtf(-rt00_2 - rt10_2 + 1.0f);
    float b1 = sqrtf(-rt01_2 - rt11_2 + 1.0f);
    const float sp = -rt00 * rt01 - rt10 * rt11;
    if (sp < 0.0f) b1 = -b1;
    for (int r = 1; r <= 3; r++) {
        r1[(r - 1) * 3 + 0] = (rt00) * RV(r, 1) + (rt10) * RV(r, 2) + (b0) * RV(r, 3);
        r1[(r - 1) * 3 + 1] = (rt01) * RV(r, 1) + (rt11) * RV(r, 2) + (b1) * RV(r, 3);
        r1[(r - 1) * 3 + 2] = (b1 * rt10 - b0 * rt11) * RV(r, 1) + (b0 * rt01 - b1 * rt00) * RV(r, 2) + (rt00 * rt11 - rt01 * rt10) * RV(r, 3);
        r2[(r - 1) * 3 + 0] = (rt00) * RV(r, 1) + (rt10) * RV(r, 2) + (-b0) * RV(r, 3);
        r2[(r - 1) * 3 + 1] = (rt01) * RV(r, 1) + (rt11) * RV(r, 2) + (-b1) * RV(r, 3);
        r2[(r - 1) * 3 + 2] = (b0 * rt11 - b1 * rt10) * RV(r, 1) + (b1 * rt00 - b0 * rt01) * RV(r, 2) + (rt00 * rt11 - rt01 * rt10) * RV(r, 3);
    }
#undef RV
}

__device__ inline void compute_translation(const float obj[12], const float pts[8], const float rot[9], float t[3]) {  // src/pose.rs:269-335
    float m11 = 4.0f, m13 = 0.0f, m22 = 4.0f, m23 = 0.0f, m31 = 0.0f, m32 = 0.0f, m33 = 0.0f;
    float atb0 = 0.0f, atb1 = 0.0f, atb2 = 0.0f;
    for (int i = 0; i < 4; i++) {
        const float ox = obj[3 * i], oy = obj[3 * i + 1];
        const float rx = rot[0] * ox + rot[1] * oy;
        const float ry = rot[3] * ox + rot[4] * oy;
        const float rz = rot[6] * ox + rot[7] * oy;
        const float a2 = -pts[2 * i], b2 = -pts[2 * i + 1];
        m13 += a2; m23 += b2; m31 += a2; m32 += b2;
        m33 += a2 * a2 + b2 * b2;
        const float bx = -a2 * rz - rx;
        const float by = -b2 * rz - ry;
        atb0 += bx; atb1 += by;
        atb2 += a2 * bx + b2 * by;
    }
    const float det_a_inv = 1.0f / (m11 * m22 * m33 - m11 * m23 * m32 - m13 * m22 * m31);
    const float s11 = m22 * m33 - m23 * m32, s12 = m13 * m32, s13 = -m13 * m22;
    const float s21 = m23 * m31, s22 = m11 * m33 - m13 * m31, s23 = -m11 * m23;
    const float s31 = -m22 * m31, s32 = -m11 * m32, s33 = m11 * m22;
    t[0] = det_a_inv * (s11 * atb0 + s12 * atb1 + s13 * atb2);
    t[1] = det_a_inv * (s21 * atb0 + s22 * atb1 + s23 * atb2);
    t[2] = det_a_inv * (s31 * atb0 + s32 * atb1 + s33 * atb2);
}

__device__ inline float reprojection_error(const a3_pose& p, const float obj[12], const float pts[8]) {  // src/pose.rs:337-348
    float error = 0.0f;
    const float* r = p.rotation;
    for (int i = 0; i < 4; i++) {
        const float x = obj[3 * i], y = obj[3 * i + 1], z = obj[3 * i + 2];
        const float px = (r[0] * x + r[1] * y + r[2] * z) + p.translation[0];
        const float py = (r[3] * x + r[4] * y + r[5] * z) + p.translation[1];
        const float pz = (r[6] * x + r[7] * y + r[8] * z) + p.translation[2];
        const float zz = pz > 1e-5f ? pz : 1e-5f;
        const float dx = (px / zz) - pts[2 * i];
        const float dy = (py / zz) - pts[2 * i + 1];
        error += sqrtf(dx * dx + dy * dy);
    }
    return error;
}

__device__ inline void solve_normalized(const float pts[8], float marker_size_mm, a3_pose* o1, a3_pose* o2) {  // src/pose.rs:64-156
    const float hw = 0.5f * marker_size_mm;
    const float obj[12] = {-hw, hw, 0.0f, hw, hw, 0.0f, hw, -hw, 0.0f, -hw, -hw, 0.0f};
    const float p1x = -pts[0], p1y = -pts[1], p2x = -pts[2], p2y = -pts[3], p3x = -pts[4], p3y = -pts[5], p4x = -pts[6], p4y = -pts[7];
    const float half_width = marker_size_mm / 2.0f;
    const float det_inv = -1.0f / (half_width * (p1x * p2y - p2x * p1y - p1x * p4y + p2x * p3y - p3x * p2y + p4x * p1y + p3x * p4y - p4x * p3y));
    float h[9];
    h[0] = det_inv * (p1x * p3x * p2y - p2x * p3x * p1y - p1x * p4x * p2y + p2x * p4x * p1y - p1x * p3x * p4y + p1x * p4x * p3y + p2x * p3x * p4y - p2x * p4x * p3y);
    h[1] = det_inv * (p1x * p2x * p3y - p1x * p3x * p2y - p1x * p2x * p4y + p2x * p4x * p1y + p1x * p3x * p4y - p3x * p4x * p1y - p2x * p4x * p3y + p3x * p4x * p2y);
    h[2] = det_inv * half_width * (p1x * p2x * p3y - p2x * p3x * p1y - p1x * p2x * p4y + p1x * p4x * p2y - p1x * p4x * p3y + p3x * p4x * p1y + p2x * p3x * p4y - p3x * p4x * p2y);
    h[3] = det_inv * (p1x * p2y * p3y - p2x * p1y * p3y - p1x * p2y * p4y + p2x * p1y * p4y - p3x * p1y * p4y + p4x * p1y * p3y + p3x * p2y * p4y - p4x * p2y * p3y);
    h[4] = det_inv * (p2x * p1y * p3y - p3x * p1y * p2y - p1x * p2y * p4y + p4x * p1y * p2y + p1x * p3y * p4y - p4x * p1y * p3y - p2x * p3y * p4y + p3x * p2y * p4y);
    h[5] = det_inv * half_width * (p1x * p2y * p3y - p3x * p1y * p2y - p2x * p1y * p4y + p4x * p1y * p2y - p1x * p3y * p4y + p3x * p1y * p4y + p2x * p3y * p4y - p4x * p2y * p3y);
    h[6] = -det_inv * (p1x * p3y - p3x * p1y - p1x * p4y - p2x * p3y + p3x * p2y + p4x * p1y + p2x * p4y - p4x * p2y);
    h[7] = det_inv * (p1x * p2y - p2x * p1y - p1x * p3y + p3x * p1y + p2x * p4y - p4x * p2y - p3x * p4y + p4x * p3y);
    h[8] = 1.0f;
    const float j[4] = {h[0] - h[6] * h[2], h[1] - h[7] * h[2], h[3] - h[6] * h[5], h[4] - h[7] * h[5]};
    a3_pose a, b;
    compute_rotations(j, h[2], h[5], a.rotation, b.rotation);
    compute_translation(obj, pts, a.rotation, a.translation);
    compute_translation(obj, pts, b.rotation, b.translation);
    a.error = reprojection_error(a, obj, pts);
    b.error = reprojection_error(b, obj, pts);
    if (a.error < b.error) { *o1 = a; *o2 = b; } else { *o1 = b; *o2 = a; }
}

}  // namespace a3
