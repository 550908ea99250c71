// The two quaternion conversions of DenseFusion/lib/transformations.py in float64, shared by the pose kernels (pose.hip) and the depth ICP
// polish (icp_polish.hip): quaternion_matrix (:1254-1278) and quaternion_from_matrix with isprecise=True (:1320-1341, :1361-1363).
// Everything here lives in the including translation unit's anonymous namespace.
#pragma once
#include "common.h"

namespace {

struct Mat4 { double m[4][4]; };

__device__ Mat4 quaternion_matrix(const double qin[4])
{
    Mat4 M;
    double q[4] = {qin[0], qin[1], qin[2], qin[3]};
    const double n = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) M.m[i][j] = i == j ? 1.0 : 0.0;
    if (n < 2.220446049250313e-16 * 4.0) return M;
    const double s = sqrt(2.0 / n);
    for (int i = 0; i < 4; ++i) q[i] *= s;
    double o[4][4];
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) o[i][j] = q[i] * q[j];
    M.m[0][0] = 1.0 - o[2][2] - o[3][3]; M.m[0][1] = o[1][2] - o[3][0]; M.m[0][2] = o[1][3] + o[2][0];
    M.m[1][0] = o[1][2] + o[3][0]; M.m[1][1] = 1.0 - o[1][1] - o[3][3]; M.m[1][2] = o[2][3] - o[1][0];
    M.m[2][0] = o[1][3] - o[2][0]; M.m[2][1] = o[2][3] + o[1][0]; M.m[2][2] = 1.0 - o[1][1] - o[2][2];
    return M;
}

__device__ void quaternion_from_matrix_precise(const Mat4& M, double q[4])
{
    const double t0 = M.m[0][0] + M.m[1][1] + M.m[2][2] + M.m[3][3];
    double t;
    if (t0 > M.m[3][3]) {
        t = t0;
        q[0] = t;
        q[3] = M.m[1][0] - M.m[0][1];
        q[2] = M.m[0][2] - M.m[2][0];
        q[1] = M.m[2][1] - M.m[1][2];
    } else {
        int i = 0, j = 1, k = 2;
        if (M.m[1][1] > M.m[0][0]) { i = 1; j = 2; k = 0; }
        if (M.m[2][2] > M.m[i][i]) { i = 2; j = 0; k = 1; }
        t = M.m[i][i] - (M.m[j][j] + M.m[k][k]) + M.m[3][3];
        double p[4];
        p[i] = t;
        p[j] = M.m[i][j] + M.m[j][i];
        p[k] = M.m[k][i] + M.m[i][k];
        p[3] = M.m[k][j] - M.m[j][k];
        q[0] = p[3]; q[1] = p[0]; q[2] = p[1]; q[3] = p[2];
    }
    const double s = 0.5 / sqrt(t * M.m[3][3]);
    for (int a = 0; a < 4; ++a) q[a] *= s;
    if (q[0] < 0.0)
        for (int a = 0; a < 4; ++a) q[a] = -q[a];
}

}  // namespace
