// Depth ICP polish of the pose stage: for every object of a batch, register its observed depth points (camera frame, what
// ape_backproject_f32 wrote) to its class's model cloud, starting from the pose the networks left, and return the polished pose with a
// fit score -- ONE launch, nothing read back, no host pointer tables: capturable in a HIP graph.
//
// Semantics per object: open3d 0.9 RegistrationICP with TransformationEstimationPointToPoint, the loop ape_icp_run_batch_f64 (kind 0,
// pointcloud.hip "ICP iteration entirely on the device") runs in three launches per iteration: evaluate (nearest model point with
// d^2 < max_dist^2, difference first, then square; ties to the lowest model index), fitness / inlier rmse, relative convergence test,
// iteration limit, fewer than 3 correspondences, else Umeyama without scale (svd3_rotation) and T <- U.T with the source moved by U.
//
// Layout: one workgroup of kPT = 1024 threads per object (16 waves: the search is a chain of dependent loads per query, so the
// iteration time is rounds-per-wave x latency-per-round -- more waves means fewer rounds, and an object needs no more than one CU).
//   * the object's observed points live in LDS as float64 (N x 24 B) and are moved in place by every update, like open3d's copy;
//   * the class's grid (sorted points, keys, order: 36 B per model point) is staged into LDS too when it fits beside them, so the
//     binary search and the cell runs of pc_grid.h's for_my_cell read LDS instead of L2; a larger model set is searched in global
//     memory by the same code;
//   * kG = 32 lanes share a query, 32 queries per round.  The 27 cells of a query are 9 runs of the sorted order (the three cells along
//     z of one (cx, cy) have consecutive keys): 18 lanes find the runs' ends by binary search (pc_grid.h's cell_of / pack_key /
//     lower_bound), then the 32 lanes split the candidates of all runs evenly -- a lane per cell, as for_my_cell has it, makes every
//     wave wait for its fullest cell (measured: 93 of 110 us per evaluation at 486 points; this form: see DESIGN.md 6zb);
//   * the 17 sums of an evaluation are taken by one wave each: lane l adds the points l, l + 64, ... in that order, then a butterfly
//     over the wave: an order that depends on the object's point count alone, hence the same bits alone and in any batch;
//   * thread 0 runs the step (3x3 SVD, composition, convergence test) between two barriers; no cross-workgroup synchronisation.
//
// The estimator is a compile-time parameter of the loop (kEst): kPointToPoint is the above; kPointToPlane is open3d's
// TransformationEstimationPointToPlane on the model's normals, the loop ape_icp_run_batch_f64 runs with kind 1 (icp_step, pointcloud.hip):
// the same search, 29 sums in p2plane_sums_kernel_body's layout -- one wave each, in the order above -- and thread 0 solves the 6x6
// normal equations (pc_grid.h's solve6) where point-to-point runs the SVD.  The normals stay in global memory ([M][3] float64 in the
// order of the cloud's points, fetched through the grid's `order`): read once per correspondence and sum, resident in L2, and 24 B more
// per model point in LDS would push a 2600-point model out of it.
#include <string>

#include "pc_grid.h"
#include "pose_quat.h"

namespace {

constexpr int kPT = 1024;             // threads per object
constexpr int kPG = kPT / kG;         // query groups per workgroup
constexpr int kNS = 17;               // [0] count, [1] sum d^2, [2..4] sum s, [5..7] sum t, [8..16] sum s_a t_b (p2p_sums_kernel_body)
constexpr int kMaxObs = 2048;         // observed points per object (36 B of LDS each: the point, its d^2, its correspondence)
constexpr int kLdsBudget = 144 * 1024;   // dynamic LDS of the kernel: 160 KB per CU minus the static arrays and some air
constexpr int kTableCols = 5;         // model_table[c] = (sorted, keys, order, origin as addresses, n)
constexpr int kPointToPoint = 0, kPointToPlane = 1;
constexpr int kNSPlane = 29;          // [0] count, [1] sum d^2, [2..22] upper triangle of J^T J (row major), [23..28] J^T r (p2plane_sums_kernel_body)

struct PolishArgs {
    const float4* pts4; const int* n_cand; const int* obj_class; const int64_t* table; const double* pose_in; double* pose_out; double* stats;
    const int64_t* ntable;            // kPointToPlane: normals_table[c] = address of class c's normals; unused (null) otherwise
    int N, n_classes, max_m, lds_model, max_iteration;
    double cell, r2, rel_fitness, rel_rmse, min_fitness;
};

// timing-only build (make variant NAME=clk SRC=icp_polish DEFS=-DAPE_POLISH_CLOCKS; results wrong): stats = 100 MHz ticks spent in the
// search, the sums and the step, and the evaluations run
#ifdef APE_POLISH_CLOCKS
#define APE_POLISH_CLK(...) __VA_ARGS__
#else
#define APE_POLISH_CLK(...)
#endif

// component k of a point-to-plane Jacobian row J = [s x n, n], in p2plane_sums_kernel_body's expressions
__device__ __forceinline__ double plane_j(const double* s, const double* nn, int k)
{
    if (k >= 3) return nn[k - 3];
    const int u = k == 2 ? 0 : k + 1, w = k == 0 ? 2 : k - 1;
    return s[u] * nn[w] - s[w] * nn[u];
}

// the loop of one object; g: the model's grid (in LDS or in global memory); src, cj, cd: the object's points, their correspondences
// (position in the grid's sorted order, -1 none) and squared distances, in LDS; nrm (kPointToPlane): the model's normals [g.n][3] in the
// order of the cloud's points, in global memory
template <int kEst>
__device__ __forceinline__ void polish_loop(const Grid& g, const double* __restrict__ nrm, double* __restrict__ src, int* __restrict__ cj, double* __restrict__ cd, int ns, const PolishArgs& a,
                                            const double* __restrict__ pin, double* __restrict__ pout, double* __restrict__ so)
{
    __shared__ double tot[kEst == kPointToPoint ? kNS : kNSPlane];
    __shared__ double Up[12];         // the pending update (rows 0..2 of a 4x4): the initial guess first, then every step's U
    __shared__ double Tm[12];         // T, camera frame -> model frame
    __shared__ double st[4];          // fitness, inlier rmse, correspondences, stop reason
    __shared__ int ctl[2];            // [0] done, [1] updates applied to T
    const int tid = threadIdx.x, lane = tid % kG, grp = tid / kG;

    if (tid == 0) {
        // init = inverse([R(q / |q|) | t]): R^T, -R^T t
        const Mat4 M = quaternion_matrix(pin);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) Tm[r * 4 + c] = M.m[c][r];
            Tm[r * 4 + 3] = -((M.m[0][r] * pin[4] + M.m[1][r] * pin[5]) + M.m[2][r] * pin[6]);
        }
        for (int k = 0; k < 12; ++k) Up[k] = Tm[k];
        st[0] = st[1] = st[2] = st[3] = 0.0;
        ctl[0] = 0; ctl[1] = 0;
    }
    __syncthreads();

    bool first = true;                // (thread 0's: no earlier evaluation to compare with)
    APE_POLISH_CLK(long long clk[3] = {0, 0, 0}; long long c0 = wall_clock64(); int evals = 0;)
    for (;;) {
        // evaluate, part 1: move every point by the pending update and find its correspondence (kG lanes per point)
        for (int i = grp; i < ns; i += kPG) {
            const double x = src[i * 3], y = src[i * 3 + 1], z = src[i * 3 + 2];
            double q[3];
            for (int r = 0; r < 3; ++r) q[r] = ((Up[r * 4] * x + Up[r * 4 + 1] * y) + Up[r * 4 + 2] * z) + Up[r * 4 + 3];
            double best = a.r2;
            unsigned bi = 0xffffffffu;
            int bj = -1;
            // the 27 cells are 9 runs of the sorted order (the three cells along z of one (cx, cy) have consecutive keys): lanes 0..8 find
            // the runs' first positions, lanes 9..17 their ends, then all kG lanes share the candidates of the 9 runs evenly
            long c[3];
            cell_of(q, g.origin, g.h, c);
            int pos = 0;
            if (lane < 18) {
                const int r = lane < 9 ? lane : lane - 9;
                const long cx = c[0] + r / 3 - 1, cy = c[1] + r % 3 - 1;
                if (cx >= 0 && cx <= 2097151 && cy >= 0 && cy <= 2097151) {
                    const long z0 = c[2] > 0 ? c[2] - 1 : 0, z1 = c[2] < 2097151 ? c[2] + 1 : 2097151;
                    pos = lower_bound(g.keys, g.n, lane < 9 ? pack_key(cx, cy, z0) : pack_key(cx, cy, z1) + 1);
                }
            }
            int lo[9], len[9], total = 0;
            for (int r = 0; r < 9; ++r) {
                lo[r] = __shfl(pos, r, kG);
                len[r] = __shfl(pos, r + 9, kG) - lo[r];
                total += len[r];
            }
            for (int k = lane; k < total; k += kG) {
                int kk = k, j = 0;
                bool placed = false;
                for (int r = 0; r < 9; ++r) {
                    if (!placed && kk < len[r]) { j = lo[r] + kk; placed = true; }
                    kk -= len[r];
                }
                const double ex = g.sorted[(size_t)j * 3] - q[0], ey = g.sorted[(size_t)j * 3 + 1] - q[1], ez = g.sorted[(size_t)j * 3 + 2] - q[2];
                const double d2 = (ex * ex + ey * ey) + ez * ez;
                const unsigned o = g.order[j];
                if (d2 < best || (d2 == best && bi != 0xffffffffu && o < bi)) { best = d2; bi = o; bj = j; }   // ties: lowest original index
            }
            for (int m = kG / 2; m >= 1; m >>= 1) {
                const double ob = __shfl_xor(best, m, kG);
                const unsigned oi = __shfl_xor(bi, m, kG);
                const int oj = __shfl_xor(bj, m, kG);
                if (oi != 0xffffffffu && (bi == 0xffffffffu || ob < best || (ob == best && oi < bi))) { best = ob; bi = oi; bj = oj; }
            }
            if (lane == 0) {
                src[i * 3] = q[0]; src[i * 3 + 1] = q[1]; src[i * 3 + 2] = q[2];
                cj[i] = bi == 0xffffffffu ? -1 : bj;
                cd[i] = best;
            }
        }
        __syncthreads();
        APE_POLISH_CLK(if (tid == 0) { const long long c1 = wall_clock64(); clk[0] += c1 - c0; c0 = c1; })
        // part 2: the 17 sums, one wave per sum (wave 0 also takes the 17th): lane l adds the points l, l + 64, ... in that order, then a
        // butterfly over the wave -- an order that depends on ns alone
        if constexpr (kEst == kPointToPoint) for (int v = tid >> 6; v < kNS; v += kPT / 64) {
            const int l = tid & 63, sa = v < 8 ? (v - 2) : (v - 8) / 3, ta = v < 8 ? (v - 5) : (v - 8) % 3;
            double w = 0.0;
            for (int i = l; i < ns; i += 64) {
                const int j = cj[i];
                if (j < 0) continue;
                double term;
                if (v == 0) term = 1.0;
                else if (v == 1) term = cd[i];
                else if (v < 5) term = src[i * 3 + sa];
                else if (v < 8) term = g.sorted[(size_t)j * 3 + ta];
                else term = src[i * 3 + sa] * g.sorted[(size_t)j * 3 + ta];
                w += term;
            }
            for (int m = 32; m >= 1; m >>= 1) w += __shfl_xor(w, m, 64);
            if (l == 0) tot[v] = w;
        }
        // point-to-plane: the 29 sums in the same order, two rounds of the 16 waves; sum v >= 2 is J_ja J_jb (the triangle row major) or
        // J_ja r, and every wave works out r and its two components of J per point -- nothing per point is kept between the sums
        if constexpr (kEst == kPointToPlane) for (int v = tid >> 6; v < kNSPlane; v += kPT / 64) {
            const int l = tid & 63;
            int ja = v >= 23 ? v - 23 : 0, jb = 0;
            if (v >= 2 && v < 23) { int k = v - 2; while (k >= 6 - ja) { k -= 6 - ja; ++ja; } jb = ja + k; }
            double w = 0.0;
            for (int i = l; i < ns; i += 64) {
                const int j = cj[i];
                if (j < 0) continue;
                double term;
                if (v == 0) term = 1.0;
                else if (v == 1) term = cd[i];
                else {
                    const double* s = src + i * 3;
                    const double* nn = nrm + (size_t)g.order[j] * 3;
                    if (v < 23) term = plane_j(s, nn, ja) * plane_j(s, nn, jb);
                    else {
                        const double* t = g.sorted + (size_t)j * 3;
                        const double r = ((s[0] - t[0]) * nn[0] + (s[1] - t[1]) * nn[1]) + (s[2] - t[2]) * nn[2];
                        term = plane_j(s, nn, ja) * r;
                    }
                }
                w += term;
            }
            for (int m = 32; m >= 1; m >>= 1) w += __shfl_xor(w, m, 64);
            if (l == 0) tot[v] = w;
        }
        __syncthreads();
        APE_POLISH_CLK(if (tid == 0) { const long long c1 = wall_clock64(); clk[1] += c1 - c0; c0 = c1; ++evals; })
        if constexpr (kEst == kPointToPoint) if (tid == 0) {
            // icp_step of pointcloud.hip, kind 0
            const double n_corr = tot[0];
            const double fitness = n_corr / (double)ns;
            const double rmse = n_corr > 0 ? sqrt(tot[1] / n_corr) : 0.0;
            const double pf = st[0], pr = st[1];
            st[0] = fitness; st[1] = rmse; st[2] = n_corr;
            if (!first && fabs(pf - fitness) < a.rel_fitness && fabs(pr - rmse) < a.rel_rmse) { ctl[0] = 1; st[3] = 1.0; }
            else if (ctl[1] >= a.max_iteration) { ctl[0] = 1; st[3] = 3.0; }
            else if (n_corr < 3.0) { ctl[0] = 1; st[3] = 2.0; }
            else {
                double mu_s[3], mu_t[3], C[3][3], R[3][3];
                for (int c = 0; c < 3; ++c) { mu_s[c] = tot[2 + c] / n_corr; mu_t[c] = tot[5 + c] / n_corr; }
                for (int c = 0; c < 3; ++c) for (int d = 0; d < 3; ++d) C[c][d] = tot[8 + d * 3 + c] / n_corr - mu_t[c] * mu_s[d];   // (1/n) sum (t - mu_t)(s - mu_s)^T
                svd3_rotation(C, R);
                double U[12], Tn[12];
                for (int c = 0; c < 3; ++c) {
                    for (int d = 0; d < 3; ++d) U[c * 4 + d] = R[c][d];
                    U[c * 4 + 3] = mu_t[c] - ((R[c][0] * mu_s[0] + R[c][1] * mu_s[1]) + R[c][2] * mu_s[2]);
                }
                for (int c = 0; c < 3; ++c)
                    for (int d = 0; d < 4; ++d)                      // row 3 of T is (0, 0, 0, 1)
                        Tn[c * 4 + d] = ((U[c * 4] * Tm[d] + U[c * 4 + 1] * Tm[4 + d]) + U[c * 4 + 2] * Tm[8 + d]) + (d == 3 ? U[c * 4 + 3] : 0.0);
                for (int k = 0; k < 12; ++k) { Tm[k] = Tn[k]; Up[k] = U[k]; }
                ctl[1] += 1;
            }
            first = false;
        }
        if constexpr (kEst == kPointToPlane) if (tid == 0) {
            // icp_step of pointcloud.hip, kind 1
            const double n_corr = tot[0];
            const double fitness = n_corr / (double)ns;
            const double rmse = n_corr > 0 ? sqrt(tot[1] / n_corr) : 0.0;
            const double pf = st[0], pr = st[1];
            st[0] = fitness; st[1] = rmse; st[2] = n_corr;
            if (!first && fabs(pf - fitness) < a.rel_fitness && fabs(pr - rmse) < a.rel_rmse) { ctl[0] = 1; st[3] = 1.0; }
            else if (ctl[1] >= a.max_iteration) { ctl[0] = 1; st[3] = 3.0; }
            else if (n_corr < 6.0) { ctl[0] = 1; st[3] = 2.0; }
            else {
                double M[6][7];
                int k = 2;
                for (int c = 0; c < 6; ++c) for (int d = c; d < 6; ++d) { M[c][d] = M[d][c] = tot[k]; ++k; }
                for (int c = 0; c < 6; ++c) M[c][6] = -tot[23 + c];
                double U[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, Tn[12];      // a singular system: the identity, and still an update
                if (solve6(M)) {
                    const double x[6] = {M[0][6], M[1][6], M[2][6], M[3][6], M[4][6], M[5][6]};
                    double R[3][3];
                    vec6_rotation(x, R);
                    for (int c = 0; c < 3; ++c) {
                        for (int d = 0; d < 3; ++d) U[c * 4 + d] = R[c][d];
                        U[c * 4 + 3] = x[3 + c];
                    }
                }
                for (int c = 0; c < 3; ++c)
                    for (int d = 0; d < 4; ++d)                      // row 3 of T is (0, 0, 0, 1)
                        Tn[c * 4 + d] = ((U[c * 4] * Tm[d] + U[c * 4 + 1] * Tm[4 + d]) + U[c * 4 + 2] * Tm[8 + d]) + (d == 3 ? U[c * 4 + 3] : 0.0);
                for (int k2 = 0; k2 < 12; ++k2) { Tm[k2] = Tn[k2]; Up[k2] = U[k2]; }
                ctl[1] += 1;
            }
            first = false;
        }
        __syncthreads();
        APE_POLISH_CLK(if (tid == 0) { const long long c1 = wall_clock64(); clk[2] += c1 - c0; c0 = c1; })
        if (ctl[0]) break;
    }

    if (tid == 0) {
        for (int k = 0; k < 4; ++k) so[k] = st[k];
        APE_POLISH_CLK(so[0] = (double)clk[0]; so[1] = (double)clk[1]; so[2] = (double)clk[2]; so[3] = (double)evals;)
        if (ctl[1] == 0 || st[0] < a.min_fitness) {
            for (int k = 0; k < 7; ++k) pout[k] = pin[k];
        } else {
            // pose_out = inverse(T) = [R^T | -R^T t], its quaternion as ape_pose_compose_f64 writes one
            Mat4 C;
            for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) C.m[r][c] = r == c ? 1.0 : 0.0;
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C.m[r][c] = Tm[c * 4 + r];
            double q[4];
            quaternion_from_matrix_precise(C, q);
            for (int k = 0; k < 4; ++k) pout[k] = q[k];
            for (int r = 0; r < 3; ++r) pout[4 + r] = -((Tm[r] * Tm[3] + Tm[4 + r] * Tm[7]) + Tm[8 + r] * Tm[11]);
        }
    }
}

template <int kEst>
__global__ __launch_bounds__(kPT) void icp_polish_kernel(const PolishArgs a)
{
    extern __shared__ double dyn[];   // observed points [N][3], d^2 [N], correspondence [N + (N & 1)], then (lds_model) sorted [max_m][3], keys [max_m], order [max_m]
    __shared__ double org[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* pin = a.pose_in + (size_t)b * 7;
    double* pout = a.pose_out + (size_t)b * 7;
    double* so = a.stats + (size_t)b * 4;
    const int nc = a.n_cand[b];
    const int ns = nc < 0 ? 0 : (nc < a.N ? nc : a.N);
    const int cls = a.obj_class[b];
    const bool known = cls >= 0 && cls < a.n_classes;
    const int64_t* row = a.table + (size_t)(known ? cls : 0) * kTableCols;
    const double* g_normals = nullptr;
    if constexpr (kEst == kPointToPlane) g_normals = known ? (const double*)(uintptr_t)a.ntable[cls] : nullptr;
    const int64_t m64 = known && (kEst == kPointToPoint || g_normals) ? row[4] : 0;       // (a class without normals: as one without points)
    if (m64 < 1 || m64 > 0x7fffffff || ns < 1) {        // (uniform over the workgroup) nothing to register: the pose passes through
        if (tid < 7) pout[tid] = pin[tid];
        if (tid < 4) so[tid] = (tid == 3 && known) ? 2.0 : 0.0;
        return;
    }
    const int m = (int)m64;
    const double* g_sorted = (const double*)(uintptr_t)row[0];
    const u64* g_keys = (const u64*)(uintptr_t)row[1];
    const unsigned* g_order = (const unsigned*)(uintptr_t)row[2];
    const double* g_origin = (const double*)(uintptr_t)row[3];

    double* src = dyn;
    double* cd = dyn + (size_t)a.N * 3;
    int* cj = (int*)(cd + a.N);
    double* model = (double*)(cj + a.N + (a.N & 1));
    const float4* p4 = a.pts4 + (size_t)b * a.N;
    for (int i = tid; i < ns; i += kPT) {               // rows from ns on are choose's wrap padding: never read
        const float4 p = p4[i];
        src[i * 3] = (double)p.x; src[i * 3 + 1] = (double)p.y; src[i * 3 + 2] = (double)p.z;
    }
    if (tid < 3) org[tid] = g_origin[tid];
    if (a.lds_model && m <= a.max_m) {
        double* l_sorted = model;
        u64* l_keys = (u64*)(l_sorted + (size_t)a.max_m * 3);
        unsigned* l_order = (unsigned*)(l_keys + a.max_m);
        for (int i = tid; i < m * 3; i += kPT) l_sorted[i] = g_sorted[i];
        for (int i = tid; i < m; i += kPT) { l_keys[i] = g_keys[i]; l_order[i] = g_order[i]; }
        __syncthreads();
        polish_loop<kEst>(Grid{l_sorted, l_keys, l_order, org, m, a.cell}, g_normals, src, cj, cd, ns, a, pin, pout, so);
    } else {
        __syncthreads();
        polish_loop<kEst>(Grid{g_sorted, g_keys, g_order, org, m, a.cell}, g_normals, src, cj, cd, ns, a, pin, pout, so);
    }
}

// the checks and the launch of both exports; `who`: the export's name for ape_last_error
template <int kEst>
int launch_polish(const char* who, int n, const float* points4, const int* n_cand, int N, const int* obj_class, const int64_t* model_table,
                  const int64_t* normals_table, int n_classes, int max_model_points, double cell, const double* pose_in, double max_dist,
                  double relative_fitness, double relative_rmse, int max_iteration, double min_fitness, double* pose_out, double* stats, void* stream)
{
    const auto refuse = [who](const char* what) { ape::set_last_error((std::string(who) + ": " + what).c_str()); return APE_EINVAL; };
    if (n < 0) return refuse("n < 0");
    if (N <= 0 || N > kMaxObs) return refuse("N must be in 1..2048");
    if (!(max_dist > 0)) return refuse("max_dist <= 0");
    if (!(cell >= max_dist)) return refuse("cell < max_dist");
    if (n_classes < 1 || max_model_points < 1 || !model_table) return refuse("empty model table");
    if (kEst == kPointToPlane && !normals_table) return refuse("no normals table");
    if (max_iteration < 0) return refuse("max_iteration < 0");
    if (n == 0) return APE_OK;
    if (!points4 || !n_cand || !obj_class || !pose_in || !pose_out || !stats) return refuse("null buffer");
    const size_t obs = (size_t)N * 32 + (size_t)(N + (N & 1)) * 4, grid = (size_t)max_model_points * 36 + 4;     // (+4: an odd count of order words keeps the total a multiple of 8)
    const int lds_model = obs + grid <= (size_t)kLdsBudget;
    const size_t lds = obs + (lds_model ? (grid & ~(size_t)7) : 0);
    static ape::DeviceOnce once;      // (one per instantiation)
    int rc = ape::device_once(once, reinterpret_cast<const void*>(icp_polish_kernel<kEst>), kLdsBudget, nullptr);
    if (rc != APE_OK) return rc;
    const PolishArgs a{(const float4*)points4, n_cand, obj_class, model_table, pose_in, pose_out, stats, normals_table, N, n_classes, max_model_points,
                       lds_model, max_iteration, cell, max_dist * max_dist, relative_fitness, relative_rmse, min_fitness};
    hipLaunchKernelGGL(icp_polish_kernel<kEst>, dim3(n), dim3(kPT), lds, (hipStream_t)stream, a);
    return ape::check_launch(who);
}

}  // namespace

/* see include/ape_hip.h */
extern "C" int ape_icp_polish_batch_f64(int n, const float* points4, const int* n_cand, int N, const int* obj_class, const int64_t* model_table,
                                        int n_classes, int max_model_points, double cell, const double* pose_in, double max_dist,
                                        double relative_fitness, double relative_rmse, int max_iteration, double min_fitness, double* pose_out,
                                        double* stats, void* stream)
{
    return launch_polish<kPointToPoint>("ape_icp_polish_batch_f64", n, points4, n_cand, N, obj_class, model_table, nullptr, n_classes, max_model_points, cell,
                                        pose_in, max_dist, relative_fitness, relative_rmse, max_iteration, min_fitness, pose_out, stats, stream);
}

/* see include/ape_hip.h */
extern "C" int ape_icp_polish_plane_batch_f64(int n, const float* points4, const int* n_cand, int N, const int* obj_class, const int64_t* model_table,
                                              const int64_t* normals_table, int n_classes, int max_model_points, double cell, const double* pose_in,
                                              double max_dist, double relative_fitness, double relative_rmse, int max_iteration, double min_fitness,
                                              double* pose_out, double* stats, void* stream)
{
    return launch_polish<kPointToPlane>("ape_icp_polish_plane_batch_f64", n, points4, n_cand, N, obj_class, model_table, normals_table, n_classes,
                                        max_model_points, cell, pose_in, max_dist, relative_fitness, relative_rmse, max_iteration, min_fitness, pose_out,
                                        stats, stream);
}
