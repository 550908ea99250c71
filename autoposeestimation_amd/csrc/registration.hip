// Global registration kernels (reference pc_reconstruction/open3d_utils.py:19-49: FPFH features of both down-sampled clouds, then RANSAC
// on feature matches before ICP), float64 like the rest of the point-cloud path, restating open3d 0.9 Feature.cpp / Registration.cpp:
//   fpfh_spfh_kernel     hybrid neighbour list of every point (d^2 < r^2, ordered by (d^2, index), first max_nn) + its SPFH histogram;
//                        the lists are kept for the second pass (see below)
//   fpfh_kernel          FPFH = per-sub-histogram normalised sum of the neighbours' SPFH weighted by 1 / d^2, plus the point's own SPFH
//   feature_nn_kernel    nearest target feature of every source feature (squared L2 over 33 dimensions, exact, ties -> lowest index):
//                        target tiles in LDS, the target range split over blockIdx.y, partial winners merged in slice order
//   ransac_hyp_kernel    one RANSAC iteration per thread (seeded splitmix64 draws, edge-length checker, Umeyama, distance checker) and
//                        an ordered in-block compaction of the passing iteration indices; ransac_append_kernel keeps the first
//                        max_validation of them in iteration order
//   ransac_validate_*    every kept hypothesis against the whole source cloud (nearest target within max_correspondence_distance through
//                        the target's grid), fixed-order sums, then the winner by (fitness desc, rmse asc, iteration asc)
//   fgr_*                fast global registration on the same features: the mutual matches in source order, the tuple test in chunks of
//                        trials (the first maximum_tuple_count passing ones in trial order), each cloud's mean and largest centred norm,
//                        and the whole Gauss-Newton optimisation of a pair in one workgroup (correspondences in LDS)
// The neighbour lists of pass 1 are written out (12 B per entry) rather than recomputed in pass 2: the selection -- min(max_nn, candidates)
// rounds of a 32-lane shuffle reduction over the candidate list -- is most of pass 1's time, and re-reading 1.2 KB per point is not.
// Every kernel is written in the batched form of pointcloud.hip ("BATCHED forms"): a by-value table of up to kMaxBatch per-pair argument
// records, the pair's index in a grid dimension, and a per-pair extent so that a block beyond its pair's extent exits.  A pair's blocks,
// partial layouts and summation orders depend on that pair's sizes alone, so its result does not depend on its slot or its neighbours.
// There are no one-pair entry points: a single pair is a call with nb = 1.
#include "common.h"
#include "pc_grid.h"

namespace {

constexpr int kT = 256;
constexpr int kGroups = kT / kG;          // queries per block in the kG-lanes-per-query kernels
constexpr int kFeatMaxNN = 128;           // largest max_nn of the FPFH search
constexpr int kFCand = 256;               // in-radius candidates a group keeps in LDS; more: the selection rounds re-walk the cells
constexpr int kBins = 33;
constexpr int kMaxRansacN = 16;
constexpr int kNNT = 128;                 // source features per block of feature_nn_kernel (one per thread)
constexpr int kNNTile = 64;               // target features per LDS tile
constexpr int kNNBlocks = 2048;           // blocks a feature_nn launch aims at (all pairs together)
constexpr int kMaxBatch = 16;             // pairs / clouds per launch, as pointcloud.hip
template <class T> struct Batch { T t[kMaxBatch]; };

using ape::align_up;

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// open3d ComputePairFeatures: f = (f0 angle, f1, f2, |d|); all zero when the points coincide or d is parallel to the chosen normal
__device__ void pair_features(const double* p1, const double* n1, const double* p2, const double* n2, double f[4])
{
    f[0] = f[1] = f[2] = f[3] = 0.0;
    double dp[3] = {p2[0] - p1[0], p2[1] - p1[1], p2[2] - p1[2]};
    const double len = sqrt(dot3(dp, dp));
    if (len == 0.0) return;
    const double a1 = dot3(n1, dp) / len, a2 = dot3(n2, dp) / len;
    const double* m1 = n1;
    const double* m2 = n2;
    double f2;
    if (acos(fabs(a1)) > acos(fabs(a2))) {
        m1 = n2; m2 = n1;
        dp[0] = -dp[0]; dp[1] = -dp[1]; dp[2] = -dp[2];
        f2 = -a2;
    } else {
        f2 = a1;
    }
    double v[3], w[3];
    cross3(dp, m1, v);
    const double vn = sqrt(dot3(v, v));
    if (vn == 0.0) return;
    v[0] /= vn; v[1] /= vn; v[2] /= vn;
    cross3(m1, v, w);
    f[3] = len;
    f[2] = f2;
    f[1] = dot3(v, m2);
    f[0] = atan2(dot3(w, m2), dot3(m1, m2));
}

__device__ __forceinline__ int bin11(double x)
{
    const double v = floor(x);
    if (!(v >= 0.0)) return 0;
    return v >= 10.0 ? 10 : (int)v;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// FPFH pass 1: kG lanes per point (as normals_kernel in pointcloud.hip).  The in-radius candidates of the 27 cells go to the group's LDS
// list; cnt = min(max_nn, candidates) rounds take the smallest (d^2, original index) after the last one taken.  Entry 0 (the point
// itself) is skipped like open3d does; every further entry adds 100 / (cnt - 1) to three bins, summed in list order by the bin's lane.
struct BFpfh { Grid g; const double* pts; const double* nrm; int* nbr; double* nbr_d2; int* nbr_cnt; double* spfh; double* out; int n, gx; };

__global__ __launch_bounds__(kT) void fpfh_spfh_kernel(const Batch<BFpfh> bt, double r2, int max_nn)
{
    const BFpfh& a = bt.t[blockIdx.y];
    if ((int)blockIdx.x >= a.gx) return;
    const Grid& g = a.g;
    const double* __restrict__ pts = a.pts;
    const double* __restrict__ nrm = a.nrm;
    int* __restrict__ nbr = a.nbr;
    double* __restrict__ nbr_d2 = a.nbr_d2;
    int* __restrict__ nbr_cnt = a.nbr_cnt;
    double* __restrict__ spfh = a.spfh;
    const int n = a.n;
    __shared__ double cand_d[kGroups][kFCand];
    __shared__ int cand_o[kGroups][kFCand];
    __shared__ int sel[kGroups][kFeatMaxNN];
    __shared__ unsigned char bins[kGroups][kFeatMaxNN][3];
    __shared__ int ncand[kGroups];
    const int lane = threadIdx.x % kG, grp = threadIdx.x / kG;
    const int i = (blockIdx.x * kT + threadIdx.x) / kG;
    const bool valid = i < n;
    if (lane == 0) ncand[grp] = 0;
    __syncthreads();
    double q[3] = {0, 0, 0};
    if (valid) {
        for (int d = 0; d < 3; ++d) q[d] = pts[(size_t)i * 3 + d];
        for_my_cell(g, q, lane, [&](int j, double d2) {
            if (d2 >= r2) return;
            const int p = atomicAdd(&ncand[grp], 1);
            if (p < kFCand) { cand_d[grp][p] = d2; cand_o[grp][p] = (int)g.order[j]; }
        });
    }
    __syncthreads();
    const int nc = ncand[grp];
    const bool listed = nc <= kFCand;
    const int cnt = valid ? (nc < max_nn ? nc : max_nn) : 0;
    double last_d = -1.0;
    int last_o = -1;
    for (int r = 0; r < cnt; ++r) {
        double bd = 1e300;
        int bo = 0x7fffffff;
        auto offer = [&](int o, double d) {
            const bool after = d > last_d || (d == last_d && o > last_o);
            if (after && (d < bd || (d == bd && o < bo))) { bd = d; bo = o; }
        };
        if (listed) for (int p = lane; p < nc; p += kG) offer(cand_o[grp][p], cand_d[grp][p]);
        else for_my_cell(g, q, lane, [&](int j, double d2) { if (d2 < r2) offer((int)g.order[j], d2); });
        for (int m = kG / 2; m >= 1; m >>= 1) {
            const double od = __shfl_xor(bd, m, kG);
            const int oo = __shfl_xor(bo, m, kG);
            if (od < bd || (od == bd && oo < bo)) { bd = od; bo = oo; }
        }
        last_d = bd; last_o = bo;
        if (lane == 0) {
            sel[grp][r] = bo;
            nbr[(size_t)i * max_nn + r] = bo;
            nbr_d2[(size_t)i * max_nn + r] = bd;
        }
    }
    if (valid && lane == 0) nbr_cnt[i] = cnt;
    __syncthreads();
    if (cnt > 1) {
        double ni[3];
        for (int d = 0; d < 3; ++d) ni[d] = nrm[(size_t)i * 3 + d];
        for (int k = 1 + lane; k < cnt; k += kG) {
            const int o = sel[grp][k];
            double f[4];
            pair_features(q, ni, pts + (size_t)o * 3, nrm + (size_t)o * 3, f);
            bins[grp][k][0] = (unsigned char)bin11(11.0 * (f[0] + M_PI) / (2.0 * M_PI));
            bins[grp][k][1] = (unsigned char)(11 + bin11(11.0 * (f[1] + 1.0) * 0.5));
            bins[grp][k][2] = (unsigned char)(22 + bin11(11.0 * (f[2] + 1.0) * 0.5));
        }
    }
    __syncthreads();
    if (valid) {
        const double incr = cnt > 1 ? 100.0 / (double)(cnt - 1) : 0.0;
        for (int b = lane; b < kBins; b += kG) {
            double h = 0.0;
            for (int k = 1; k < cnt; ++k) if (bins[grp][k][b / 11] == b) h += incr;
            spfh[(size_t)i * kBins + b] = h;
        }
    }
}

// FPFH pass 2: lane b sums SPFH_k[b] / d^2_k over the list in order (d^2 = 0 skipped), each 11-bin block is scaled to 100, then SPFH_i is
// added.  Points with at most one list entry get zeros.
__global__ __launch_bounds__(kT) void fpfh_kernel(const Batch<BFpfh> bt, int max_nn)
{
    const BFpfh& a = bt.t[blockIdx.y];
    if ((int)blockIdx.x >= a.gx) return;
    const int* __restrict__ nbr = a.nbr;
    const double* __restrict__ nbr_d2 = a.nbr_d2;
    const int* __restrict__ nbr_cnt = a.nbr_cnt;
    const double* __restrict__ spfh = a.spfh;
    double* __restrict__ out = a.out;
    const int n = a.n;
    __shared__ double F[kGroups][kBins];
    const int lane = threadIdx.x % kG, grp = threadIdx.x / kG;
    const int i = (blockIdx.x * kT + threadIdx.x) / kG;
    const bool valid = i < n;
    const int cnt = valid ? nbr_cnt[i] : 0;
    for (int b = lane; b < kBins; b += kG) {
        double acc = 0.0;
        for (int k = 1; k < cnt; ++k) {
            const double d = nbr_d2[(size_t)i * max_nn + k];
            if (d == 0.0) continue;
            acc += spfh[(size_t)nbr[(size_t)i * max_nn + k] * kBins + b] / d;
        }
        F[grp][b] = acc;
    }
    __syncthreads();
    if (!valid) return;
    for (int b = lane; b < kBins; b += kG) {
        double v = 0.0;
        if (cnt > 1) {
            const int b0 = b / 11 * 11;
            double s = 0.0;
            for (int j = 0; j < 11; ++j) s += F[grp][b0 + j];
            const double sc = s != 0.0 ? 100.0 / s : 0.0;
            v = F[grp][b] * sc + spfh[(size_t)i * kBins + b];
        }
        out[(size_t)i * kBins + b] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// nearest feature: blockIdx.z = pair, blockIdx.y takes target slice [y * slice, min(nt, (y + 1) * slice)); d = sum_j (a_j - b_j)^2 in j
// order; strict < in ascending target order keeps the lowest index of a tie, and so does the slice-ordered merge -- the minimum and its
// lowest index do not depend on where the slices are cut, so the slice count is free to follow the size of the whole launch
struct BNN { const double* src; const double* tgt; double* part_d; int* part_i; int* nn; int ns, nt, slice, nslice, gx; };

__global__ __launch_bounds__(kNNT) void feature_nn_kernel(const Batch<BNN> bt)
{
    const BNN& p = bt.t[blockIdx.z];
    if ((int)blockIdx.x >= p.gx || (int)blockIdx.y >= p.nslice) return;
    const double* __restrict__ src = p.src;
    const double* __restrict__ tgt = p.tgt;
    double* __restrict__ part_d = p.part_d;
    int* __restrict__ part_i = p.part_i;
    const int ns = p.ns, nt = p.nt, slice = p.slice;
    __shared__ double tile[kNNTile][kBins];
    const int s = blockIdx.x * kNNT + threadIdx.x;
    const bool valid = s < ns;
    double a[kBins];
#pragma unroll
    for (int j = 0; j < kBins; ++j) a[j] = valid ? src[(size_t)s * kBins + j] : 0.0;
    const int t0 = blockIdx.y * slice;
    const int t1 = min(nt, t0 + slice);
    double best = INFINITY;
    int bi = -1;
    for (int tb = t0; tb < t1; tb += kNNTile) {
        const int m = min(kNNTile, t1 - tb);
        __syncthreads();
        for (int e = threadIdx.x; e < m * kBins; e += kNNT) tile[e / kBins][e % kBins] = tgt[(size_t)tb * kBins + e];
        __syncthreads();
        if (!valid) continue;
        for (int k = 0; k < m; ++k) {
            double d = 0.0;
#pragma unroll
            for (int j = 0; j < kBins; ++j) { const double e = a[j] - tile[k][j]; d += e * e; }
            if (d < best) { best = d; bi = tb + k; }
        }
    }
    if (valid) { part_d[(size_t)blockIdx.y * ns + s] = best; part_i[(size_t)blockIdx.y * ns + s] = bi; }
}

__global__ void feature_nn_merge_kernel(const Batch<BNN> bt)
{
    const BNN& p = bt.t[blockIdx.y];
    const double* __restrict__ part_d = p.part_d;
    const int* __restrict__ part_i = p.part_i;
    int* __restrict__ nn = p.nn;
    const int ns = p.ns, nslice = p.nslice;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < ns; s += gridDim.x * blockDim.x) {
        double best = part_d[s];
        int bi = part_i[s];
        for (int y = 1; y < nslice; ++y) {
            const double d = part_d[(size_t)y * ns + s];
            if (d < best) { best = d; bi = part_i[(size_t)y * ns + s]; }
        }
        nn[s] = bi;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// RANSAC (open3d 0.9 RegistrationRANSACBasedOnFeatureMatching with a seeded sampler instead of rand())
struct Hyp {
    const double* src; int ns;
    const double* tgt; int nt;
    const int* nn;              // [ns] nearest target feature of every source feature
    int ransac_n;
    u64 seed;
    double edge_sim;            // < 0: no edge-length checker
    double dist_thr;            // < 0: no distance checker
};

__device__ __forceinline__ u64 splitmix64(u64 x)
{
    u64 z = x + 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// iteration `it`: draw, check, estimate; T[12] = rows 0..2 of the 4x4.  With checks = false only the draw and the estimate run (the
// validation recomputes the transformations of the kept iterations this way)
__device__ bool ransac_hypothesis(const Hyp& h, int it, bool checks, double T[12])
{
    int s[kMaxRansacN], t[kMaxRansacN];
    const int rn = h.ransac_n;
    for (int j = 0; j < rn; ++j) {
        s[j] = (int)(splitmix64((h.seed << 32) ^ (u64)((long long)it * rn + j)) % (u64)h.ns);
        t[j] = h.nn[s[j]];
        if (t[j] < 0 || t[j] >= h.nt) return false;
    }
    if (checks && h.edge_sim >= 0.0)                     // CorrespondenceCheckerBasedOnEdgeLength: every pair of edges
        for (int a = 0; a < rn; ++a)
            for (int b = a + 1; b < rn; ++b) {
                const double* sa = h.src + (size_t)s[a] * 3; const double* sb = h.src + (size_t)s[b] * 3;
                const double* ta = h.tgt + (size_t)t[a] * 3; const double* tb = h.tgt + (size_t)t[b] * 3;
                const double es[3] = {sa[0] - sb[0], sa[1] - sb[1], sa[2] - sb[2]}, et[3] = {ta[0] - tb[0], ta[1] - tb[1], ta[2] - tb[2]};
                const double ds = sqrt(dot3(es, es)), dt = sqrt(dot3(et, et));
                if (ds < dt * h.edge_sim || dt < ds * h.edge_sim) return false;
            }
    // Eigen::umeyama without scaling: C = (1/n) sum (t - mu_t)(s - mu_s)^T, R from its SVD, t = mu_t - R mu_s
    double mu_s[3] = {0, 0, 0}, mu_t[3] = {0, 0, 0};
    for (int j = 0; j < rn; ++j)
        for (int d = 0; d < 3; ++d) { mu_s[d] += h.src[(size_t)s[j] * 3 + d]; mu_t[d] += h.tgt[(size_t)t[j] * 3 + d]; }
    for (int d = 0; d < 3; ++d) { mu_s[d] /= (double)rn; mu_t[d] /= (double)rn; }
    double C[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, R[3][3];
    for (int j = 0; j < rn; ++j) {
        double es[3], et[3];
        for (int d = 0; d < 3; ++d) { es[d] = h.src[(size_t)s[j] * 3 + d] - mu_s[d]; et[d] = h.tgt[(size_t)t[j] * 3 + d] - mu_t[d]; }
        for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) C[a][b] += et[a] * es[b];
    }
    for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) C[a][b] /= (double)rn;
    svd3_rotation(C, R);
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) T[a * 4 + b] = R[a][b];
        T[a * 4 + 3] = mu_t[a] - ((R[a][0] * mu_s[0] + R[a][1] * mu_s[1]) + R[a][2] * mu_s[2]);
    }
    if (checks && h.dist_thr >= 0.0)                     // CorrespondenceCheckerBasedOnDistance: |t - T s| <= thr for every pair
        for (int j = 0; j < rn; ++j) {
            const double* p = h.src + (size_t)s[j] * 3;
            const double* q = h.tgt + (size_t)t[j] * 3;
            double e[3];
            for (int a = 0; a < 3; ++a) e[a] = q[a] - (((T[a * 4] * p[0] + T[a * 4 + 1] * p[1]) + T[a * 4 + 2] * p[2]) + T[a * 4 + 3]);
            if (sqrt(dot3(e, e)) > h.dist_thr) return false;
        }
    return true;
}

// iterations [it0, it0 + n_it) of pair blockIdx.y: block b writes its passing iterations in order to blist[b][0..bcount[b]); a no-op once
// the pair's own n_kept word is full (the other pairs of the launch go on)
struct BHyp { Hyp h; int* kept; int* n_kept; int* blist; int* bcount; };

__global__ __launch_bounds__(kT) void ransac_hyp_kernel(const Batch<BHyp> bt, int it0, int n_it, int max_validation)
{
    const BHyp& a = bt.t[blockIdx.y];
    if (*a.n_kept >= max_validation) return;
    const Hyp& h = a.h;
    int* __restrict__ blist = a.blist;
    int* __restrict__ bcount = a.bcount;
    __shared__ int wc[kT / 64];
    const int gid = blockIdx.x * kT + threadIdx.x;
    double T[12];
    const bool pass = gid < n_it && ransac_hypothesis(h, it0 + gid, true, T);
    const unsigned long long m = __ballot(pass);
    const int wave = threadIdx.x / 64, wl = threadIdx.x % 64;
    if (wl == 0) wc[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < kT / 64; ++w) { off += w < wave ? wc[w] : 0; tot += wc[w]; }
    if (pass) blist[(size_t)blockIdx.x * kT + off + __popcll(m & ((1ULL << wl) - 1ULL))] = it0 + gid;
    if (threadIdx.x == 0) bcount[blockIdx.x] = tot;
}

// one block per pair: appends the blocks' lists in block order to kept[*n_kept ..] up to max_validation entries
__global__ __launch_bounds__(kT) void ransac_append_kernel(const Batch<BHyp> bt, int nb, int max_validation)
{
    const BHyp& a = bt.t[blockIdx.y];
    const int* __restrict__ blist = a.blist;
    const int* __restrict__ bcount = a.bcount;
    int* __restrict__ kept = a.kept;
    int* __restrict__ n_kept = a.n_kept;
    const int base = *n_kept;
    if (base >= max_validation) return;
    __shared__ int pre[kT + 1];
    const int per = (nb + kT - 1) / kT;
    const int b0 = min(nb, (int)threadIdx.x * per), b1 = min(nb, b0 + per);
    int s = 0;
    for (int b = b0; b < b1; ++b) s += bcount[b];
    pre[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int k = 0; k < kT; ++k) { const int v = pre[k]; pre[k] = run; run += v; }
        pre[kT] = run;
    }
    __syncthreads();
    int off = base + pre[threadIdx.x];
    for (int b = b0; b < b1 && off < max_validation; ++b) {
        const int c = bcount[b];
        for (int r = 0; r < c && off + r < max_validation; ++r) kept[off + r] = blist[(size_t)b * kT + r];
        off += c;
    }
    __syncthreads();
    if (threadIdx.x == 0) *n_kept = min(max_validation, base + pre[kT]);
}

struct BVal { Grid g; Hyp h; const int* kept; double* T12; double* part; double* fr; double* out; int nh, G; };

// the transformation of every kept iteration (rows 0..2)
__global__ void ransac_models_kernel(const Batch<BVal> bt)
{
    const BVal& a = bt.t[blockIdx.y];
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.nh) return;
    double T[12];
    ransac_hypothesis(a.h, a.kept[k], false, T);
    for (int e = 0; e < 12; ++e) a.T12[(size_t)k * 12 + e] = T[e];
}

// blockIdx.z = pair, blockIdx.y = hypothesis, blockIdx.x < G (the pair's own count) strides over the source (kGroups points per pass, kG
// lanes each, as nn1_group_kernel); the group's lane 0 accumulates its points' count / sum d^2 in order, the block reduces its groups
// in order -> part[h][bx][2]
__global__ __launch_bounds__(kT) void ransac_validate_kernel(const Batch<BVal> bt, double r2)
{
    const BVal& a = bt.t[blockIdx.z];
    const int G = a.G;
    if ((int)blockIdx.x >= G || (int)blockIdx.y >= a.nh) return;
    const Grid& g = a.g;
    const double* __restrict__ src = a.h.src;
    double* __restrict__ part = a.part;
    const int ns = a.h.ns;
    __shared__ double sc[kGroups], sd[kGroups];
    const int lane = threadIdx.x % kG, grp = threadIdx.x / kG;
    const double* T = a.T12 + (size_t)blockIdx.y * 12;
    double cnt = 0.0, sum = 0.0;
    for (int base = blockIdx.x * kGroups; base < ns; base += G * kGroups) {
        const int i = base + grp;
        if (i >= ns) continue;
        const double x = src[(size_t)i * 3], y = src[(size_t)i * 3 + 1], z = src[(size_t)i * 3 + 2];
        double q[3];
        for (int r = 0; r < 3; ++r) q[r] = ((T[r * 4] * x + T[r * 4 + 1] * y) + T[r * 4 + 2] * z) + T[r * 4 + 3];
        double best = r2;
        bool found = false;
        for_my_cell(g, q, lane, [&](int, double d2) { if (d2 < best) { best = d2; found = true; } });
        for (int m = kG / 2; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best, m, kG);
            const int of = __shfl_xor((int)found, m, kG);
            if (of && (!found || ob < best)) { best = ob; found = true; }
        }
        if (found) { cnt += 1.0; sum += best; }
    }
    if (lane == 0) { sc[grp] = cnt; sd[grp] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double c = 0.0, s = 0.0;
        for (int k = 0; k < kGroups; ++k) { c += sc[k]; s += sd[k]; }
        part[((size_t)blockIdx.y * G + blockIdx.x) * 2] = c;
        part[((size_t)blockIdx.y * G + blockIdx.x) * 2 + 1] = s;
    }
}

// one block per pair: fitness / rmse of every hypothesis (partials summed in block order), then the winner in iteration order, replaced only by a
// strictly better one (open3d IsBetterRANSACThan) starting from (identity, 0, 0).  out: [0..15] T, [16] fitness, [17] rmse,
// [18] correspondences, [19] winner's position in `kept` (-1: none), [20] its iteration index (-1: none)
__global__ __launch_bounds__(kT) void ransac_select_kernel(const Batch<BVal> bt)
{
    const BVal& a = bt.t[blockIdx.y];
    const double* __restrict__ part = a.part;
    const double* __restrict__ T12 = a.T12;
    const int* __restrict__ kept = a.kept;
    double* __restrict__ fr = a.fr;
    double* __restrict__ out = a.out;
    const int G = a.G, nh = a.nh, ns = a.h.ns;
    for (int k = threadIdx.x; k < nh; k += kT) {
        double c = 0.0, s = 0.0;
        for (int b = 0; b < G; ++b) { c += part[((size_t)k * G + b) * 2]; s += part[((size_t)k * G + b) * 2 + 1]; }
        fr[(size_t)k * 3] = c / (double)ns;
        fr[(size_t)k * 3 + 1] = c > 0.0 ? sqrt(s / c) : 0.0;
        fr[(size_t)k * 3 + 2] = c;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double bf = 0.0, br = 0.0, bc = 0.0;
    int bk = -1;
    for (int k = 0; k < nh; ++k) {
        const double f = fr[(size_t)k * 3], r = fr[(size_t)k * 3 + 1];
        if (f > bf || (f == bf && r < br)) { bf = f; br = r; bc = fr[(size_t)k * 3 + 2]; bk = k; }
    }
    for (int e = 0; e < 16; ++e) out[e] = (e % 5 == 0) ? 1.0 : 0.0;
    if (bk >= 0) for (int e = 0; e < 12; ++e) out[e] = T12[(size_t)bk * 12 + e];
    out[16] = bf; out[17] = br; out[18] = bc; out[19] = bk; out[20] = bk >= 0 ? (double)kept[bk] : -1.0;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Fast global registration (Zhou, Park, Koltun, ECCV 2016; open3d 0.9 FastGlobalRegistration.cpp restated).
// fgr_mutual_kernel: one block per pair walks the source in kT-sized steps and keeps, in ascending i, the pairs (i, nn_st[i]) whose
// match points back (nn_ts[nn_st[i]] == i) -- the ordered in-block compaction of ransac_hyp_kernel with a running base.
struct BMut { const int* nn_st; const int* nn_ts; int* ms; int* mt; int* n_mutual; int ns, nt; };

__global__ __launch_bounds__(kT) void fgr_mutual_kernel(const Batch<BMut> bt)
{
    const BMut& a = bt.t[blockIdx.x];
    const int* __restrict__ nn_st = a.nn_st;
    const int* __restrict__ nn_ts = a.nn_ts;
    const int ns = a.nt > 0 ? a.ns : 0, nt = a.nt;
    __shared__ int wc[kT / 64];
    const int wave = threadIdx.x / 64, wl = threadIdx.x % 64;
    int base = 0;
    for (int i0 = 0; i0 < ns; i0 += kT) {
        const int i = i0 + threadIdx.x;
        int j = -1;
        bool pass = false;
        if (i < ns) {
            j = nn_st[i];
            pass = j >= 0 && j < nt && nn_ts[j] == i;
        }
        const unsigned long long m = __ballot(pass);
        __syncthreads();
        if (wl == 0) wc[wave] = __popcll(m);
        __syncthreads();
        int off = 0, tot = 0;
        for (int w = 0; w < kT / 64; ++w) { off += w < wave ? wc[w] : 0; tot += wc[w]; }
        if (pass) {
            const int o = base + off + __popcll(m & ((1ULL << wl) - 1ULL));
            a.ms[o] = i;
            a.mt[o] = j;
        }
        base += tot;
    }
    if (threadIdx.x == 0) *a.n_mutual = base;
}

// the tuple test: trial t draws three positions of the mutual list (the RANSAC sampler's form) and passes when every edge of the source
// triangle and its target twin are within tuple_scale of each other, both ways, strictly.  Trials [t0, t0 + n_t) of pair blockIdx.y,
// below the pair's own limit of 100 * ncorr; the passing trial indices go to blist / bcount exactly as ransac_hyp_kernel's, and
// ransac_append_kernel keeps the first max_tuples of them
struct BTup { const double* src; const double* tgt; const int* ms; const int* mt; const int* n_mutual; const int* n_kept; int* blist; int* bcount; u64 seed; int lim; };   // lim = min(ns, nt): a count beyond it is not a mutual list's

__device__ __forceinline__ int fgr_draw(u64 seed, int t, int k, int ncorr)
{
    return (int)(splitmix64((seed << 32) ^ (u64)(3LL * t + k)) % (u64)ncorr);
}

__global__ __launch_bounds__(kT) void fgr_tuple_kernel(const Batch<BTup> bt, int t0, int n_t, int max_tuples, double tuple_scale)
{
    const BTup& a = bt.t[blockIdx.y];
    if (*a.n_kept >= max_tuples) return;
    const double* __restrict__ src = a.src;
    const double* __restrict__ tgt = a.tgt;
    const int ncorr = *a.n_mutual;
    __shared__ int wc[kT / 64];
    const int gid = blockIdx.x * kT + threadIdx.x;
    bool pass = false;
    if (gid < n_t && ncorr > 0 && ncorr <= a.lim && (long long)t0 + gid < 100LL * ncorr) {
        int si[3], ti[3];
        for (int k = 0; k < 3; ++k) {
            const int r = fgr_draw(a.seed, t0 + gid, k, ncorr);
            si[k] = a.ms[r];
            ti[k] = a.mt[r];
        }
        pass = true;
        for (int k = 0; k < 3; ++k) {
            const double* sa = src + (size_t)si[k] * 3; const double* sb = src + (size_t)si[(k + 1) % 3] * 3;
            const double* ta = tgt + (size_t)ti[k] * 3; const double* tb = tgt + (size_t)ti[(k + 1) % 3] * 3;
            const double es[3] = {sa[0] - sb[0], sa[1] - sb[1], sa[2] - sb[2]}, et[3] = {ta[0] - tb[0], ta[1] - tb[1], ta[2] - tb[2]};
            const double li = sqrt(dot3(es, es)), lj = sqrt(dot3(et, et));
            if (!(li * tuple_scale < lj && lj * tuple_scale < li)) pass = false;
        }
    }
    const unsigned long long m = __ballot(pass);
    const int wave = threadIdx.x / 64, wl = threadIdx.x % 64;
    if (wl == 0) wc[wave] = __popcll(m);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < kT / 64; ++w) { off += w < wave ? wc[w] : 0; tot += wc[w]; }
    if (pass) a.blist[(size_t)blockIdx.x * kT + off + __popcll(m & ((1ULL << wl) - 1ULL))] = t0 + gid;
    if (threadIdx.x == 0) a.bcount[blockIdx.x] = tot;
}

// mean and largest centred norm of one cloud: blockIdx.x = 0 source / 1 target, blockIdx.y = pair; thread t sums points t, t + kT, ... in
// order, the block folds the kT partials by a halving tree -> norm8[x * 4 ..] = (mean[3], max |p - mean|); zeros for an empty cloud
struct BCen { const double* pts[2]; int n[2]; double* norm8; };

__global__ __launch_bounds__(kT) void fgr_center_kernel(const Batch<BCen> bt)
{
    const BCen& a = bt.t[blockIdx.y];
    const double* __restrict__ p = a.pts[blockIdx.x];
    const int n = a.n[blockIdx.x];
    __shared__ double sh[3][kT];
    double s[3] = {0, 0, 0};
    for (int i = threadIdx.x; i < n; i += kT) for (int d = 0; d < 3; ++d) s[d] += p[(size_t)i * 3 + d];
    for (int d = 0; d < 3; ++d) sh[d][threadIdx.x] = s[d];
    __syncthreads();
    for (int m = kT / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) for (int d = 0; d < 3; ++d) sh[d][threadIdx.x] += sh[d][threadIdx.x + m];
        __syncthreads();
    }
    double mu[3];
    for (int d = 0; d < 3; ++d) mu[d] = n > 0 ? sh[d][0] / (double)n : 0.0;
    __syncthreads();
    double mx = 0.0;
    for (int i = threadIdx.x; i < n; i += kT) {
        const double e[3] = {p[(size_t)i * 3] - mu[0], p[(size_t)i * 3 + 1] - mu[1], p[(size_t)i * 3 + 2] - mu[2]};
        const double v = sqrt(dot3(e, e));
        if (v > mx) mx = v;
    }
    sh[0][threadIdx.x] = mx;
    __syncthreads();
    for (int m = kT / 2; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m && sh[0][threadIdx.x + m] > sh[0][threadIdx.x]) sh[0][threadIdx.x] = sh[0][threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* out = a.norm8 + blockIdx.x * 4;
        out[0] = mu[0]; out[1] = mu[1]; out[2] = mu[2]; out[3] = sh[0][0];
    }
}

// x = -(L D L^T)^-1 b without pivoting; false at the first pivot that is not finite and positive
__device__ bool fgr_ldlt_solve(const double A[6][6], const double b[6], double x[6])
{
    double L[6][6], D[6];
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
        if (!(d > 0.0) || !(d < INFINITY)) return false;
        D[j] = d;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i][j];
            for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * D[k];
            L[i][j] = v / d;
        }
    }
    double y[6];
    for (int i = 0; i < 6; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= L[i][k] * y[k];
        y[i] = v;
    }
    for (int i = 0; i < 6; ++i) y[i] /= D[i];
    for (int i = 5; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
        x[i] = v;
    }
    for (int i = 0; i < 6; ++i) x[i] = -x[i];
    return true;
}

// The whole optimisation of pair blockIdx.x in one workgroup.  The correspondences (three per kept trial, re-drawn from the trial index)
// are loaded once into LDS as (p target, q source), centred and scaled, one row per coordinate; a thread owns entries t, t + kT, ... for the whole loop, so the
// list needs no barrier.  An iteration: every thread adds its entries' 27 sums (upper triangle of JTJ, then JTr) in entry order, a wave
// folds its 64 lanes by a butterfly of shuffles (every lane ends with the same bits), thread 0 adds the kT / 64 wave totals in wave order,
// solves by LDL^T and builds the update (TransformVector6dToMatrix4d), and all threads move their q.  Nothing is written to global memory
// before the end.  out[24]: [0..15] T in the clouds' own units, [16] iterations run, [17] scale, [18] the last par, [19] correspondences
struct BFgr { const double* src; const double* tgt; const int* ms; const int* mt; const int* n_mutual; const int* kept; const double* norm8; double* out; u64 seed; int ns, nt, nk; };

constexpr int kFgrMaxCorr = 3000;

__global__ __launch_bounds__(kT) void fgr_optimize_kernel(const Batch<BFgr> bt, int use_absolute_scale, int decrease_mu, double division_factor,
                                                          double max_corr_dist, int n_iter)
{
    extern __shared__ __attribute__((aligned(16))) double fgr_pq[];          // [6][nc]: p.xyz then q.xyz, a row per coordinate, so that
                                                                             // the lanes of a wave touch consecutive doubles
    __shared__ double wsum[kT / 64][27];
    __shared__ double delta[12];
    __shared__ int ok;
    const BFgr& a = bt.t[blockIdx.x];
    const double* __restrict__ nm = a.norm8;
    double* __restrict__ out = a.out;
    const int nc = 3 * a.nk;
    const int ncorr = *a.n_mutual;
    const double scale = nm[3] > nm[7] ? nm[3] : nm[7];
    const double sg = use_absolute_scale ? 1.0 : scale;
    double par = use_absolute_scale ? scale : 1.0;
    if (nc < 10 || ncorr < 1 || ncorr > a.ns || ncorr > a.nt) {              // too few correspondences: the identity
        if (threadIdx.x == 0) {
            for (int e = 0; e < 16; ++e) out[e] = (e % 5 == 0) ? 1.0 : 0.0;
            out[16] = 0.0; out[17] = scale; out[18] = par; out[19] = (double)nc;
        }
        return;
    }
    for (int c = threadIdx.x; c < nc; c += kT) {
        const int r = fgr_draw(a.seed, a.kept[c / 3], c % 3, ncorr);
        const int i = a.ms[r], j = a.mt[r];
        for (int d = 0; d < 3; ++d) {
            fgr_pq[d * nc + c] = (a.tgt[(size_t)j * 3 + d] - nm[4 + d]) / sg;
            fgr_pq[(3 + d) * nc + c] = (a.src[(size_t)i * 3 + d] - nm[d]) / sg;
        }
    }
    double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};                     // thread 0's: rows 0..2 of the normalised transformation
    const int wave = threadIdx.x / 64, wl = threadIdx.x % 64;
    int it = 0;
    for (; it < n_iter; ++it) {
        if (decrease_mu && it % 4 == 0 && par > max_corr_dist) par /= division_factor;
        double acc[27];
#pragma unroll
        for (int v = 0; v < 27; ++v) acc[v] = 0.0;
        for (int c = threadIdx.x; c < nc; c += kT) {
            const double* e = fgr_pq + c;
            const double q[3] = {e[3 * nc], e[4 * nc], e[5 * nc]};
            const double r[3] = {e[0] - q[0], e[nc] - q[1], e[2 * nc] - q[2]};
            const double w = par / (dot3(r, r) + par);
            const double s = w * w;
            const double J[3][6] = {{0.0, -q[2], q[1], -1.0, 0.0, 0.0}, {q[2], 0.0, -q[0], 0.0, -1.0, 0.0}, {-q[1], q[0], 0.0, 0.0, 0.0, -1.0}};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                int v = 0;
#pragma unroll
                for (int x = 0; x < 6; ++x) {
                    const double sj = s * J[k][x];
#pragma unroll
                    for (int y = x; y < 6; ++y) { acc[v] += sj * J[k][y]; ++v; }
                    acc[21 + x] += sj * r[k];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < 27; ++v) {
            double t = acc[v];
            for (int m = 32; m >= 1; m >>= 1) t += __shfl_xor(t, m, 64);
            if (wl == 0) wsum[wave][v] = t;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double A[6][6], b[6], x[6];
            int v = 0;
            for (int p = 0; p < 6; ++p)
                for (int q = p; q < 6; ++q) {
                    double t = wsum[0][v];
                    for (int w = 1; w < kT / 64; ++w) t += wsum[w][v];
                    A[p][q] = A[q][p] = t;
                    ++v;
                }
            for (int p = 0; p < 6; ++p) {
                double t = wsum[0][21 + p];
                for (int w = 1; w < kT / 64; ++w) t += wsum[w][21 + p];
                b[p] = t;
            }
            const bool solved = fgr_ldlt_solve(A, b, x);
            if (solved) {
                const double cx = cos(x[0]), sx = sin(x[0]), cy = cos(x[1]), sy = sin(x[1]), cz = cos(x[2]), sz = sin(x[2]);
                // TransformVector6dToMatrix4d: R = Rz(x2) Ry(x1) Rx(x0), as icp_step in pointcloud.hip
                const double Rx[3][3] = {{1, 0, 0}, {0, cx, -sx}, {0, sx, cx}}, Ry[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}}, Rz[3][3] = {{cz, -sz, 0}, {sz, cz, 0}, {0, 0, 1}};
                double T1[3][3], U[12], Tn[12];
                for (int p = 0; p < 3; ++p) for (int q = 0; q < 3; ++q) T1[p][q] = (Rz[p][0] * Ry[0][q] + Rz[p][1] * Ry[1][q]) + Rz[p][2] * Ry[2][q];
                for (int p = 0; p < 3; ++p) {
                    for (int q = 0; q < 3; ++q) U[p * 4 + q] = (T1[p][0] * Rx[0][q] + T1[p][1] * Rx[1][q]) + T1[p][2] * Rx[2][q];
                    U[p * 4 + 3] = x[3 + p];
                }
                for (int p = 0; p < 3; ++p)
                    for (int q = 0; q < 4; ++q)
                        Tn[p * 4 + q] = ((U[p * 4] * T[q] + U[p * 4 + 1] * T[4 + q]) + U[p * 4 + 2] * T[8 + q]) + (q == 3 ? U[p * 4 + 3] : 0.0);
                for (int e = 0; e < 12; ++e) { T[e] = Tn[e]; delta[e] = U[e]; }
            }
            ok = solved ? 1 : 0;
        }
        __syncthreads();
        if (!ok) break;
        for (int c = threadIdx.x; c < nc; c += kT) {
            double* e = fgr_pq + c;
            const double x = e[3 * nc], y = e[4 * nc], z = e[5 * nc];
            for (int p = 0; p < 3; ++p) e[(3 + p) * nc] = ((delta[p * 4] * x + delta[p * 4 + 1] * y) + delta[p * 4 + 2] * z) + delta[p * 4 + 3];
        }
    }
    if (threadIdx.x == 0) {                                                  // original scale: R kept, t = sg t_norm + mean_t - R mean_s
        for (int p = 0; p < 3; ++p) {
            for (int q = 0; q < 3; ++q) out[p * 4 + q] = T[p * 4 + q];
            out[p * 4 + 3] = (sg * T[p * 4 + 3] + nm[4 + p]) - ((T[p * 4] * nm[0] + T[p * 4 + 1] * nm[1]) + T[p * 4 + 2] * nm[2]);
        }
        out[12] = 0.0; out[13] = 0.0; out[14] = 0.0; out[15] = 1.0;
        out[16] = (double)it; out[17] = scale; out[18] = par; out[19] = (double)nc;
    }
}

int validate_blocks(int ns)
{
    const int g = ape::ceil_div(ns, kGroups);
    return g < 1 ? 1 : (g > 64 ? 64 : g);
}

// slices of one pair's target range when `live` pairs share the launch: the launch as a whole aims at kNNBlocks blocks
int nn_slices(int ns, int nt, int live)
{
    const int bx = ape::ceil_div(ns, kNNT);
    const int max_s = ape::ceil_div(nt, kNNTile);
    const int s = ape::ceil_div(ape::ceil_div(kNNBlocks, live < 1 ? 1 : live), bx);
    return s < 1 ? 1 : (s > max_s ? max_s : s);
}

size_t fpfh_ws(int n, int max_nn)
{
    if (n < 1) n = 1;
    if (max_nn < 1) max_nn = 1;
    return align_up((size_t)n * max_nn * 4) + align_up((size_t)n * max_nn * 8) + align_up((size_t)n * 4) + align_up((size_t)n * kBins * 8);
}

size_t nn_ws(int ns, int nt, int live)
{
    if (ns < 1) ns = 1;
    if (nt < 1) nt = 1;
    const size_t s = (size_t)nn_slices(ns, nt, live);
    return align_up(s * ns * 8) + align_up(s * ns * 4);
}

size_t ransac_ws(int ns, int chunk, int max_validation)
{
    if (ns < 1) ns = 1;
    if (chunk < 1) chunk = 1;
    if (max_validation < 1) max_validation = 1;
    const size_t nb = (size_t)ape::ceil_div(chunk, kT);
    return align_up(nb * kT * 4) + align_up(nb * 4) + align_up((size_t)max_validation * 12 * 8) +
           align_up((size_t)max_validation * validate_blocks(ns) * 2 * 8) + align_up((size_t)max_validation * 3 * 8);
}

int live_pairs(int nb, const int* ns, const int* nt)
{
    int live = 0;
    for (int c = 0; c < nb; ++c) live += (ns[c] > 0 && nt[c] > 0) ? 1 : 0;
    return live;
}

// ---- the launch code behind the entry points: nb records each (a single pair or cloud is nb = 1) -----------------------------------------
// both FPFH passes of nb clouds (g[c].n points each, 0: skipped); workspace: the clouds' fpfh_ws regions one after the other
int fpfh_launch(int nb, const Grid* g, const double* const* pts, const double* const* nrm, double radius, int max_nn, double* const* feature,
                void* ws, size_t ws_bytes, hipStream_t st, const char* what)
{
    size_t need = 0;
    for (int c = 0; c < nb; ++c) need += fpfh_ws(g[c].n, max_nn);
    if (ws_bytes < need) return APE_EWORKSPACE;
    Batch<BFpfh> b{};
    char* p = (char*)ws;
    int mg = 0;
    for (int c = 0; c < nb; ++c) {
        const int n = g[c].n;
        const size_t m = (size_t)(n < 1 ? 1 : n);
        int* nbr = (int*)p;          p += align_up(m * max_nn * 4);
        double* nbr_d2 = (double*)p; p += align_up(m * max_nn * 8);
        int* cnt = (int*)p;          p += align_up(m * 4);
        double* spfh = (double*)p;   p += align_up(m * kBins * 8);
        const int gx = n > 0 ? ape::ceil_div((long)n * kG, (long)kT) : 0;
        b.t[c] = BFpfh{g[c], pts[c], nrm[c], nbr, nbr_d2, cnt, spfh, feature[c], n, gx};
        mg = gx > mg ? gx : mg;
    }
    if (mg == 0) return APE_OK;
    hipLaunchKernelGGL(fpfh_spfh_kernel, dim3(mg, nb), dim3(kT), 0, st, b, radius * radius, max_nn);
    hipLaunchKernelGGL(fpfh_kernel, dim3(mg, nb), dim3(kT), 0, st, b, max_nn);
    return ape::check_launch(what);
}

// nearest target feature for nb (source, target) feature pairs (a pair with ns or nt == 0 is skipped); workspace: the pairs' nn_ws regions
int nn_launch(int nb, const double* const* src, const int* ns, const double* const* tgt, const int* nt, int* const* nn, void* ws, size_t ws_bytes,
              hipStream_t st, const char* what)
{
    const int live = live_pairs(nb, ns, nt);
    if (live == 0) return APE_OK;
    size_t need = 0;
    for (int c = 0; c < nb; ++c) need += (ns[c] > 0 && nt[c] > 0) ? nn_ws(ns[c], nt[c], live) : 0;
    if (ws_bytes < need) return APE_EWORKSPACE;
    Batch<BNN> b{};
    char* p = (char*)ws;
    int mgx = 0, mgy = 0, mgm = 0;
    for (int c = 0; c < nb; ++c) {
        if (ns[c] <= 0 || nt[c] <= 0) continue;              // the zeroed record: gx = nslice = ns = 0
        const int nslice0 = nn_slices(ns[c], nt[c], live);
        const int slice = ape::ceil_div(ape::ceil_div(nt[c], nslice0), kNNTile) * kNNTile;
        const int nslice = ape::ceil_div(nt[c], slice);
        double* part_d = (double*)p;
        int* part_i = (int*)(p + align_up((size_t)nslice0 * ns[c] * 8));
        p += nn_ws(ns[c], nt[c], live);
        const int gx = ape::ceil_div(ns[c], kNNT);
        const int gm = ape::ceil_div(ns[c], kT) > 1024 ? 1024 : ape::ceil_div(ns[c], kT);
        b.t[c] = BNN{src[c], tgt[c], part_d, part_i, nn[c], ns[c], nt[c], slice, nslice, gx};
        mgx = gx > mgx ? gx : mgx;
        mgy = nslice > mgy ? nslice : mgy;
        mgm = gm > mgm ? gm : mgm;
    }
    hipLaunchKernelGGL(feature_nn_kernel, dim3(mgx, mgy, nb), dim3(kNNT), 0, st, b);
    hipLaunchKernelGGL(feature_nn_merge_kernel, dim3(mgm, nb), dim3(kT), 0, st, b);
    return ape::check_launch(what);
}

// one chunk of iterations for nb pairs; kept[c] / n_kept[c] on the device; workspace: the pairs' ransac_ws(ns, n_it, max_validation) regions
int hyp_launch(int nb, const Hyp* h, int it_begin, int n_it, int max_validation, int* const* kept, int* const* n_kept, void* ws, size_t ws_bytes,
               hipStream_t st, const char* what)
{
    if (n_it == 0) return APE_OK;
    size_t need = 0;
    for (int c = 0; c < nb; ++c) need += ransac_ws(h[c].ns, n_it, max_validation);
    if (ws_bytes < need) return APE_EWORKSPACE;
    const int nblk = ape::ceil_div(n_it, kT);
    Batch<BHyp> b{};
    char* p = (char*)ws;
    for (int c = 0; c < nb; ++c) {
        b.t[c] = BHyp{h[c], kept[c], n_kept[c], (int*)p, (int*)(p + align_up((size_t)nblk * kT * 4))};
        p += ransac_ws(h[c].ns, n_it, max_validation);
    }
    hipLaunchKernelGGL(ransac_hyp_kernel, dim3(nblk, nb), dim3(kT), 0, st, b, it_begin, n_it, max_validation);
    hipLaunchKernelGGL(ransac_append_kernel, dim3(1, nb), dim3(kT), 0, st, b, nblk, max_validation);
    return ape::check_launch(what);
}

// models, validation and selection of nb pairs (nk[c] kept iterations, host counts); workspace: the pairs' ransac_ws(ns, 1, max(nk, 1))
// regions; fr[c] (may be NULL): the caller's [nk][3] array instead of the workspace's
int validate_launch(int nb, const Grid* g, const Hyp* h, const int* const* kept, const int* nk, double max_dist, double* result, double* const* fr,
                    void* ws, size_t ws_bytes, hipStream_t st, const char* what)
{
    size_t need = 0;
    for (int c = 0; c < nb; ++c) need += ransac_ws(h[c].ns, 1, nk[c]);
    if (ws_bytes < need) return APE_EWORKSPACE;
    Batch<BVal> b{};
    char* base = (char*)ws;
    int mh = 0, mG = 0;
    for (int c = 0; c < nb; ++c) {
        const int mv = nk[c] < 1 ? 1 : nk[c];
        const int G = validate_blocks(h[c].ns);
        char* p = base + align_up((size_t)kT * 4) + align_up(4);
        double* T12 = (double*)p;  p += align_up((size_t)mv * 12 * 8);
        double* part = (double*)p; p += align_up((size_t)mv * G * 2 * 8);
        b.t[c] = BVal{g[c], h[c], kept[c], T12, part, fr && fr[c] ? fr[c] : (double*)p, result + (size_t)c * 24, nk[c], G};
        base += ransac_ws(h[c].ns, 1, nk[c]);
        mh = nk[c] > mh ? nk[c] : mh;
        mG = G > mG ? G : mG;
    }
    if (mh > 0) {
        hipLaunchKernelGGL(ransac_models_kernel, dim3(ape::ceil_div(mh, 64), nb), dim3(64), 0, st, b);
        hipLaunchKernelGGL(ransac_validate_kernel, dim3(mG, mh, nb), dim3(kT), 0, st, b, max_dist * max_dist);
    }
    hipLaunchKernelGGL(ransac_select_kernel, dim3(1, nb), dim3(kT), 0, st, b);
    return ape::check_launch(what);
}

size_t fgr_ws(int chunk)
{
    const size_t nb = (size_t)ape::ceil_div(chunk < 1 ? 1 : chunk, kT);
    return align_up(nb * kT * 4) + align_up(nb * 4);
}

}  // namespace

#define APE_BATCH_CHECK(nb) if ((nb) < 1 || (nb) > kMaxBatch) return APE_EINVAL

extern "C" size_t ape_fpfh_batch_workspace_bytes(int nb, const int* n_host, int max_nn)
{
    size_t s = 0;
    for (int c = 0; n_host && c < nb && c < kMaxBatch; ++c) s += fpfh_ws(n_host[c], max_nn);
    return s;
}

extern "C" int ape_fpfh_batch_f64(int nb, BGRID_ARGS, const double* const* pts, const double* const* normals, double radius, int max_nn,
                                  double* const* feature, void* ws, size_t ws_bytes, void* stream)
{
    APE_BATCH_CHECK(nb);
    if (!sorted || !keys || !order || !origin3 || !gn || !pts || !normals || !feature || !ws || !(radius > 0) || radius > cell || max_nn < 1 ||
        max_nn > kFeatMaxNN)
        return APE_EINVAL;
    Grid g[kMaxBatch];
    for (int c = 0; c < nb; ++c) {
        if (gn[c] < 0 || (gn[c] > 0 && (!sorted[c] || !keys[c] || !order[c] || !origin3[c] || !pts[c] || !normals[c] || !feature[c]))) return APE_EINVAL;
        g[c] = BGRID(c);
    }
    return fpfh_launch(nb, g, pts, normals, radius, max_nn, feature, ws, ws_bytes, (hipStream_t)stream, "ape_fpfh_batch_f64");
}

extern "C" size_t ape_feature_nn1_batch_workspace_bytes(int nb, const int* ns_host, const int* nt_host)
{
    if (!ns_host || !nt_host || nb < 1 || nb > kMaxBatch) return 0;
    const int live = live_pairs(nb, ns_host, nt_host);
    size_t s = 0;
    for (int c = 0; c < nb; ++c) s += (ns_host[c] > 0 && nt_host[c] > 0) ? nn_ws(ns_host[c], nt_host[c], live) : 0;
    return s;
}

extern "C" int ape_feature_nn1_batch_f64(int nb, const double* const* src_feature, const int* ns, const double* const* tgt_feature, const int* nt,
                                         int* const* nn, void* ws, size_t ws_bytes, void* stream)
{
    APE_BATCH_CHECK(nb);
    if (!src_feature || !ns || !tgt_feature || !nt || !nn) return APE_EINVAL;
    for (int c = 0; c < nb; ++c) {
        if (ns[c] < 0 || nt[c] < 0) return APE_EINVAL;
        if (ns[c] > 0 && nt[c] > 0 && (!src_feature[c] || !tgt_feature[c] || !nn[c] || !ws)) return APE_EINVAL;
    }
    return nn_launch(nb, src_feature, ns, tgt_feature, nt, nn, ws, ws_bytes, (hipStream_t)stream, "ape_feature_nn1_batch_f64");
}

extern "C" size_t ape_ransac_batch_workspace_bytes(int nb, const int* ns_host, int chunk, int max_validation)
{
    size_t s = 0;
    for (int c = 0; ns_host && c < nb && c < kMaxBatch; ++c) s += ransac_ws(ns_host[c], chunk, max_validation);
    return s;
}

extern "C" int ape_ransac_hypotheses_batch_f64(int nb, const double* const* src, const int* ns, const double* const* tgt, const int* nt,
                                               const int* const* nn, int ransac_n, const long* seed_host, double edge_sim, double dist_thr,
                                               int it_begin, int n_it, int max_validation, int* kept, int* n_kept, void* ws, size_t ws_bytes,
                                               void* stream)
{
    APE_BATCH_CHECK(nb);
    if (!src || !ns || !tgt || !nt || !nn || !seed_host || !kept || !n_kept || !ws || ransac_n < 3 || ransac_n > kMaxRansacN || it_begin < 0 ||
        n_it < 0 || max_validation < 1)
        return APE_EINVAL;
    Hyp h[kMaxBatch];
    int* kp[kMaxBatch];
    int* np[kMaxBatch];
    for (int c = 0; c < nb; ++c) {
        if (!src[c] || !tgt[c] || !nn[c] || ns[c] < 1 || nt[c] < 1) return APE_EINVAL;
        h[c] = Hyp{src[c], ns[c], tgt[c], nt[c], nn[c], ransac_n, (u64)seed_host[c], edge_sim, dist_thr};
        kp[c] = kept + (size_t)c * max_validation;
        np[c] = n_kept + c;
    }
    return hyp_launch(nb, h, it_begin, n_it, max_validation, kp, np, ws, ws_bytes, (hipStream_t)stream, "ape_ransac_hypotheses_batch_f64");
}

extern "C" int ape_ransac_validate_batch_f64(int nb, BGRID_ARGS, const double* const* src, const int* ns, const double* const* tgt, const int* nt,
                                             const int* const* nn, int ransac_n, const long* seed_host, const int* kept, int kept_stride,
                                             const int* n_kept_host, double max_dist, double* result, double* const* fit_rmse, void* ws,
                                             size_t ws_bytes, void* stream)
{
    APE_BATCH_CHECK(nb);
    if (!sorted || !keys || !order || !origin3 || !gn || !src || !ns || !tgt || !nt || !nn || !seed_host || !kept || !n_kept_host || !result || !ws ||
        ransac_n < 3 || ransac_n > kMaxRansacN || kept_stride < 1 || !(max_dist > 0) || max_dist > cell)
        return APE_EINVAL;
    Grid g[kMaxBatch];
    Hyp h[kMaxBatch];
    const int* kp[kMaxBatch];
    for (int c = 0; c < nb; ++c) {
        if (!sorted[c] || !keys[c] || !order[c] || !origin3[c] || !src[c] || !tgt[c] || !nn[c] || gn[c] < 1 || ns[c] < 1 || nt[c] != gn[c] ||
            n_kept_host[c] < 0 || n_kept_host[c] > 65535 || n_kept_host[c] > kept_stride)
            return APE_EINVAL;
        g[c] = BGRID(c);
        h[c] = Hyp{src[c], ns[c], tgt[c], nt[c], nn[c], ransac_n, (u64)seed_host[c], -1.0, -1.0};
        kp[c] = kept + (size_t)c * kept_stride;
    }
    return validate_launch(nb, g, h, kp, n_kept_host, max_dist, result, fit_rmse, ws, ws_bytes, (hipStream_t)stream, "ape_ransac_validate_batch_f64");
}

// ---- fast global registration ---------------------------------------------------------------------------------------------------------
extern "C" size_t ape_fgr_workspace_bytes(int nb, int chunk)
{
    if (nb < 1 || nb > kMaxBatch) return 0;
    return (size_t)nb * fgr_ws(chunk);
}

extern "C" int ape_fgr_mutual_batch(int nb, const int* const* nn_st, const int* ns, const int* const* nn_ts, const int* nt, int* const* mutual_s,
                                    int* const* mutual_t, int* n_mutual, void* stream)
{
    APE_BATCH_CHECK(nb);
    if (!nn_st || !ns || !nn_ts || !nt || !mutual_s || !mutual_t || !n_mutual) return APE_EINVAL;
    Batch<BMut> b{};
    for (int c = 0; c < nb; ++c) {
        if (ns[c] < 0 || nt[c] < 0) return APE_EINVAL;
        const bool on = ns[c] > 0 && nt[c] > 0;
        if (on && (!nn_st[c] || !nn_ts[c] || !mutual_s[c] || !mutual_t[c])) return APE_EINVAL;
        b.t[c] = BMut{nn_st[c], nn_ts[c], mutual_s[c], mutual_t[c], n_mutual + c, on ? ns[c] : 0, on ? nt[c] : 0};
    }
    hipLaunchKernelGGL(fgr_mutual_kernel, dim3(nb), dim3(kT), 0, (hipStream_t)stream, b);
    return ape::check_launch("ape_fgr_mutual_batch");
}

extern "C" int ape_fgr_tuples_batch_f64(int nb, const double* const* src, const int* ns, const double* const* tgt, const int* nt,
                                        const int* const* mutual_s, const int* const* mutual_t, const int* n_mutual, const long* seed_host,
                                        double tuple_scale, int trial_begin, int n_trials, int max_tuples, int* kept, int* n_kept, void* ws,
                                        size_t ws_bytes, void* stream)
{
    APE_BATCH_CHECK(nb);
    if (!src || !ns || !tgt || !nt || !mutual_s || !mutual_t || !n_mutual || !seed_host || !kept || !n_kept || !ws || trial_begin < 0 ||
        n_trials < 0 || trial_begin > 0x7fffffff - n_trials || max_tuples < 1)
        return APE_EINVAL;
    if (n_trials == 0) return APE_OK;
    if (ws_bytes < (size_t)nb * fgr_ws(n_trials)) return APE_EWORKSPACE;
    const int nblk = ape::ceil_div(n_trials, kT);
    Batch<BTup> b{};
    Batch<BHyp> ba{};
    char* p = (char*)ws;
    for (int c = 0; c < nb; ++c) {
        if (ns[c] < 0 || nt[c] < 0) return APE_EINVAL;
        const int lim = ns[c] < nt[c] ? ns[c] : nt[c];
        if (lim > 0 && (!src[c] || !tgt[c] || !mutual_s[c] || !mutual_t[c])) return APE_EINVAL;
        int* blist = (int*)p;
        int* bcount = (int*)(p + align_up((size_t)nblk * kT * 4));
        p += fgr_ws(n_trials);
        b.t[c] = BTup{src[c], tgt[c], mutual_s[c], mutual_t[c], n_mutual + c, n_kept + c, blist, bcount, (u64)seed_host[c], lim};
        ba.t[c] = BHyp{Hyp{}, kept + (size_t)c * max_tuples, n_kept + c, blist, bcount};
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fgr_tuple_kernel, dim3(nblk, nb), dim3(kT), 0, st, b, trial_begin, n_trials, max_tuples, tuple_scale);
    hipLaunchKernelGGL(ransac_append_kernel, dim3(1, nb), dim3(kT), 0, st, ba, nblk, max_tuples);
    return ape::check_launch("ape_fgr_tuples_batch_f64");
}

extern "C" int ape_fgr_optimize_batch_f64(int nb, const double* const* src, const int* ns, const double* const* tgt, const int* nt,
                                          const int* const* mutual_s, const int* const* mutual_t, const int* n_mutual, const long* seed_host,
                                          const int* kept, int kept_stride, const int* n_kept_host, int use_absolute_scale, int decrease_mu,
                                          double division_factor, double max_corr_dist, int iteration_number, double* norm8, double* result,
                                          void* stream)
{
    APE_BATCH_CHECK(nb);
    if (!src || !ns || !tgt || !nt || !mutual_s || !mutual_t || !n_mutual || !seed_host || !kept || !n_kept_host || !norm8 || !result ||
        kept_stride < 1 || iteration_number < 0)
        return APE_EINVAL;
    Batch<BCen> bc{};
    Batch<BFgr> b{};
    int mk = 0;
    for (int c = 0; c < nb; ++c) {
        if (ns[c] < 0 || nt[c] < 0 || n_kept_host[c] < 0 || n_kept_host[c] > kept_stride || 3 * n_kept_host[c] > kFgrMaxCorr) return APE_EINVAL;
        const bool on = ns[c] > 0 && nt[c] > 0;
        if (on && (!src[c] || !tgt[c] || !mutual_s[c] || !mutual_t[c])) return APE_EINVAL;
        if (!on && n_kept_host[c] > 0) return APE_EINVAL;
        bc.t[c] = BCen{{src[c], tgt[c]}, {ns[c], nt[c]}, norm8 + (size_t)c * 8};
        b.t[c] = BFgr{src[c], tgt[c], mutual_s[c], mutual_t[c], n_mutual + c, kept + (size_t)c * kept_stride, norm8 + (size_t)c * 8,
                      result + (size_t)c * 24, (u64)seed_host[c], ns[c], nt[c], n_kept_host[c]};
        mk = n_kept_host[c] > mk ? n_kept_host[c] : mk;
    }
    static std::atomic<unsigned long long> attr_devs{0};                   // the dynamic-LDS attribute is per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return APE_ELAUNCH;
    if (!(attr_devs.load(std::memory_order_relaxed) >> dev & 1ULL)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(fgr_optimize_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kFgrMaxCorr * 6 * 8) != hipSuccess)
            return APE_ELAUNCH;
        attr_devs.fetch_or(1ULL << dev, std::memory_order_relaxed);
    }
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fgr_center_kernel, dim3(2, nb), dim3(kT), 0, st, bc);
    hipLaunchKernelGGL(fgr_optimize_kernel, dim3(nb), dim3(kT), (size_t)(mk < 1 ? 1 : mk) * 3 * 6 * 8, st, b, use_absolute_scale, decrease_mu, division_factor,
                       max_corr_dist, iteration_number);
    return ape::check_launch("ape_fgr_optimize_batch_f64");
}
