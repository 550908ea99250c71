// Device helpers shared by the point-cloud kernels (pointcloud.hip) and the global-registration kernels (registration.hip): the uniform
// search grid over a cloud sorted by cell key (27-cell walk, kG lanes per query), the 3x3 rotation of Eigen::umeyama without scaling, and
// -- shared with the depth ICP polish (icp_polish.hip) -- the 6x6 solve and the rotation of the point-to-plane update.
// Everything here lives in the including translation unit's anonymous namespace.
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 pack_key(long cx, long cy, long cz) { return ((u64)cx << 42) | ((u64)cy << 21) | (u64)cz; }

// key of the cell of p for a grid with origin o and cell size h (coordinates clamped into [0, 2^21))
__device__ __forceinline__ void cell_of(const double* p, const double* o, double h, long c[3])
{
    for (int d = 0; d < 3; ++d) {
        long v = (long)floor((p[d] - o[d]) / h);   // the same division keys_kernel_body uses => identical cell borders
        c[d] = v < 0 ? 0 : (v > 2097151 ? 2097151 : v);
    }
}

struct Grid {
    const double* sorted;   // [n][3] points in key order
    const u64* keys;        // [n] sorted
    const unsigned* order;  // [n] original index of sorted position
    const double* origin;   // [3]
    int n;
    double h;
};

// a Grid as the arguments of an extern "C" entry point (GRID_ARGS -> MAKE_GRID: `Grid g`), and the per-cloud arrays of the batched entry
// points (BGRID_ARGS -> BGRID(c): cloud c's Grid)
#define GRID_ARGS const double* sorted, const unsigned long long* keys, const unsigned* order, const double* origin3, int n, double cell
#define MAKE_GRID Grid g{sorted, (const u64*)keys, order, origin3, n, cell}
#define BGRID_ARGS const double* const* sorted, const unsigned long long* const* keys, const unsigned* const* order, const double* const* origin3, const int* gn, double cell
#define BGRID(c) Grid{sorted[c], (const u64*)keys[c], order[c], origin3[c], gn[c], cell}

__device__ __forceinline__ int lower_bound(const u64* keys, int n, u64 k)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (keys[mid] < k) lo = mid + 1; else hi = mid; }
    return lo;
}

// Cooperative form for the small clouds of the label path (10^4 points: one query per lane leaves most of the chip idle and every
// lane walks 27 cells through dependent loads): kG = 32 lanes share a query, lane l < 27 takes cell l of the 3x3x3 block -- one binary
// search and a short run of points -- and the group reduces with shuffles.
constexpr int kG = 32;

template <class F>
__device__ __forceinline__ void for_my_cell(const Grid& g, const double* q, int lane, F f)
{
    long c[3];
    cell_of(q, g.origin, g.h, c);
    if (lane >= 27) return;
    const long cx = c[0] + lane / 9 - 1, cy = c[1] + (lane / 3) % 3 - 1, cz = c[2] + lane % 3 - 1;
    if (cx < 0 || cx > 2097151 || cy < 0 || cy > 2097151 || cz < 0 || cz > 2097151) return;
    const u64 key = pack_key(cx, cy, cz);
    for (int j = lower_bound(g.keys, g.n, key); j < g.n && g.keys[j] == key; ++j) {
        const double ex = g.sorted[(size_t)j * 3] - q[0], ey = g.sorted[(size_t)j * 3 + 1] - q[1], ez = g.sorted[(size_t)j * 3 + 2] - q[2];
        f(j, (ex * ex + ey * ey) + ez * ez);
    }
}

__device__ void svd3_rotation(const double C[3][3], double R[3][3])
{
    // R = U diag(1, 1, det(U) det(V)) V^T for C = U S V^T (Eigen::umeyama without scaling).  One-sided (Hestenes) Jacobi: rotate
    // column pairs of A = C until orthogonal: A V' = U S.
    double A[3][3], V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) A[i][j] = C[i][j];
    for (int sweep = 0; sweep < 30; ++sweep) {
        double off = 0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double alpha = 0, beta = 0, gamma = 0;
                for (int k = 0; k < 3; ++k) { alpha += A[k][p] * A[k][p]; beta += A[k][q] * A[k][q]; gamma += A[k][p] * A[k][q]; }
                if (gamma == 0.0 || fabs(gamma) <= 1e-17 * sqrt(alpha * beta)) continue;
                off += fabs(gamma);
                const double zeta = (beta - alpha) / (2.0 * gamma);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / sqrt(1.0 + t * t), sn = c * t;
                for (int k = 0; k < 3; ++k) {
                    const double ap = A[k][p], aq = A[k][q];
                    A[k][p] = c * ap - sn * aq; A[k][q] = sn * ap + c * aq;
                    const double vp = V[k][p], vq = V[k][q];
                    V[k][p] = c * vp - sn * vq; V[k][q] = sn * vp + c * vq;
                }
            }
        if (off == 0.0) break;
    }
    double sig[3];
    for (int j = 0; j < 3; ++j) sig[j] = sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    int ord[3] = {0, 1, 2};                               // descending singular values
    for (int a = 0; a < 2; ++a) for (int b2 = a + 1; b2 < 3; ++b2) if (sig[ord[b2]] > sig[ord[a]]) { const int t = ord[a]; ord[a] = ord[b2]; ord[b2] = t; }
    double U[3][3], W[3][3];
    for (int j = 0; j < 3; ++j) {
        const int o = ord[j];
        for (int k = 0; k < 3; ++k) { W[k][j] = V[k][o]; U[k][j] = sig[o] > 0 ? A[k][o] / sig[o] : 0.0; }
    }
    if (!(sig[ord[0]] > 0)) {                             // zero covariance (all pairs coincide with their centroids): no rotation to find
        for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[i][j] = i == j ? 1.0 : 0.0;
        return;
    }
    const double tiny = 1e-13 * sig[ord[0]];
    if (sig[ord[1]] <= tiny) {                            // rank <= 1: complete U with any orthonormal pair
        double e[3] = {fabs(U[0][0]) < 0.9 ? 1.0 : 0.0, fabs(U[0][0]) < 0.9 ? 0.0 : 1.0, 0.0};
        double d = e[0] * U[0][0] + e[1] * U[1][0] + e[2] * U[2][0];
        double n2 = 0;
        for (int k = 0; k < 3; ++k) { e[k] -= d * U[k][0]; n2 += e[k] * e[k]; }
        for (int k = 0; k < 3; ++k) U[k][1] = e[k] / sqrt(n2);
    }
    if (sig[ord[2]] <= tiny) {                            // rank 2: third left vector = u0 x u1
        U[0][2] = U[1][0] * U[2][1] - U[2][0] * U[1][1];
        U[1][2] = U[2][0] * U[0][1] - U[0][0] * U[2][1];
        U[2][2] = U[0][0] * U[1][1] - U[1][0] * U[0][1];
    }
    auto det3 = [](const double M[3][3]) {
        return M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0]) + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]);
    };
    const double s33 = det3(U) * det3(W) < 0 ? -1.0 : 1.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = (U[i][0] * W[j][0] + U[i][1] * W[j][1]) + s33 * U[i][2] * W[j][2];
}

__device__ bool solve6(double M[6][7])
{
    // Gaussian elimination with partial pivoting on the augmented system (numpy.linalg.solve = LAPACK gesv); false when exactly singular
    for (int c = 0; c < 6; ++c) {
        int piv = c;
        for (int r = c + 1; r < 6; ++r) if (fabs(M[r][c]) > fabs(M[piv][c])) piv = r;
        if (M[piv][c] == 0.0) return false;
        if (piv != c) for (int k = 0; k < 7; ++k) { const double t = M[c][k]; M[c][k] = M[piv][k]; M[piv][k] = t; }
        for (int r = c + 1; r < 6; ++r) {
            const double f = M[r][c] / M[c][c];
            for (int k = c; k < 7; ++k) M[r][k] -= f * M[c][k];
        }
    }
    for (int r = 5; r >= 0; --r) {
        double v = M[r][6];
        for (int k = r + 1; k < 6; ++k) v -= M[r][k] * M[k][6];
        M[r][6] = v / M[r][r];
    }
    return true;
}

// rotation of open3d's TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0)
__device__ __forceinline__ void vec6_rotation(const double x[6], double R[3][3])
{
    const double cx = cos(x[0]), sx = sin(x[0]), cy = cos(x[1]), sy = sin(x[1]), cz = cos(x[2]), sz = sin(x[2]);
    const double Rx[3][3] = {{1, 0, 0}, {0, cx, -sx}, {0, sx, cx}}, Ry[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}}, Rz[3][3] = {{cz, -sz, 0}, {sz, cz, 0}, {0, 0, 1}};
    double T1[3][3];
    for (int a = 0; a < 3; ++a) for (int b2 = 0; b2 < 3; ++b2) T1[a][b2] = (Rz[a][0] * Ry[0][b2] + Rz[a][1] * Ry[1][b2]) + Rz[a][2] * Ry[2][b2];
    for (int a = 0; a < 3; ++a) for (int b2 = 0; b2 < 3; ++b2) R[a][b2] = (T1[a][0] * Rx[0][b2] + T1[a][1] * Rx[1][b2]) + T1[a][2] * Rx[2][b2];
}

}  // namespace
