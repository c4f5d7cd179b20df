// Polynomial-kernel sums of the Kernel Inception Distance (Binkowski et al. 2018, "Demystifying MMD GANs"):
//     k(a, b) = (a.b / d + 1)^3        Sxx = sum_{i != j} k(x_i, x_j)    Syy = sum_{i != j} k(y_i, y_j)    Sxy = sum_{i, j} k(x_i, y_j)
// for MANY groups of rows in one launch pair -- the 100 random subsets of the KID estimate, or the 80 classes of a per-class
// run -- from fp32 feature rows that never leave the device.  No Gram matrix is written: a workgroup forms one 64 x 64 block of
// dot products in fp64 on v_mfma_f64_16x16x4_f64 (rows_tile.h; every fp32 x fp32 product is exact in fp64),
// applies the kernel to its accumulator registers and keeps ONE number.
//
// Work list.  Group g contributes three segments (xx, yy, xy) in that order; a symmetric segment of T = ceil(n / 64) row tiles
// lists only the T (T + 1) / 2 tiles with tn >= tm -- strictly-upper tiles count twice, diagonal tiles once with i == j
// masked -- and an xy segment lists ceil(n / 64) x ceil(m / 64) tiles.  The host writes one 48-byte record per segment with
// the segment's first tile number; workgroup b finds its segment by bisection over those numbers and decodes (tm, tn)
// arithmetically, so the grid is exactly the number of tiles: a 40-row class costs 3 workgroups beside a 1000-row subset's 528.
//
// Reproducible by construction: no floating-point atomics.  A thread adds its 16 values in register order, the wave folds with
// a fixed butterfly, the workgroup adds its four waves in order and writes partial[tile]; the second kernel (one workgroup per
// segment) adds the segment's partials -- thread t takes tiles t, t + 256, ... in order, then a fixed tree -- and writes the sum.
// Neither order depends on where a row came from, only on its place in the group.
//
// Gaussian kernel (CMMD: Jayasumana et al. 2024, "Rethinking FID"; tise_mmd_rbf_grouped).  The same work list, tile and reductions
// with another epilogue,
//     k(a, b) = exp(-gamma d2(a, b)),      d2(a, b) = max(0, (|a|^2 + |b|^2) - 2 a.b)
// d2 is rows_tile.h's rows_d2, the function csrc/knn.hip calls: a.b from the tile, |.|^2 from rows_norm2_kernel into the
// workspace, one double per group position of each side, so that d2 of a pair is the same bits whichever side each row is
// on.  A row that holds a NaN or an infinity has the norm NaN and the clamp keeps a NaN (rows_tile.h): every kernel
// value of a pair with it is NaN, so the sums that involve the row are NaN and no other sum of the launch moves.  exp is the
// fp64 library function.  Its cost against the tile's MFMA work has not been measured.
//
// Kernels
//   mmd_tiles_kernel<MMD_POLY3>   bound: fp64 MFMA for d in the thousands (64 * 64 * 2 * d flop per tile against 2 * 64 * d * 4
//                                 bytes fetched, mostly from L2: the rows of a group are shared by all its tiles)
//   mmd_tiles_kernel<MMD_RBF>     the same tile + 16 fp64 exp per thread; bound: not measured
//   rows_norm2_kernel             (rows_tile.h) one wave per group position; bound: HBM (reads the rows once)
//   mmd_reduce_kernel             bound: latency (8 bytes per tile)
#include <vector>
#include "common.h"
#include "rows_tile.h"

struct MmdSeg {
    int64_t a0, b0;     // first row (contiguous form) or first index entry (indexed form) of the A / B side's group
    int na, nb;         // rows of the group on the A / B side
    int tile0, ntiles;  // this segment's slice of the tile list
    int kind;           // 0 = xx, 1 = yy, 2 = xy
    int tcols;          // column tiles: ceil(nb / 64)
    int pad[2];
};

enum { MMD_POLY3 = 0, MMD_RBF = 1 };

// what the Gaussian epilogue needs beside the tile: |.|^2 of group position p of a side at norm[p - first position of that side]
struct MmdRbf {
    const double* nx;
    const double* ny;
    int64_t x0, y0;
    double gamma;
};

template <int KF>
__global__ __launch_bounds__(256, 2) void mmd_tiles_kernel(const float* __restrict__ X, int64_t ldx,
                                                           const int64_t* __restrict__ ix, const float* __restrict__ Y,
                                                           int64_t ldy, const int64_t* __restrict__ iy, int d,
                                                           const MmdSeg* __restrict__ segs, int nseg,
                                                           double* __restrict__ partial, MmdRbf rbf) {
    __shared__ __attribute__((aligned(16))) float lds[GT_ROWS_LDS_FLOATS];
    const int bid = blockIdx.x;
    // the last segment whose first tile is <= bid (empty segments share their successor's number and are passed over)
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].tile0 <= bid) lo = mid; else hi = mid - 1;
    }
    const MmdSeg sg = segs[lo];
    int t = bid - sg.tile0;
    if (t >= sg.ntiles) return;                               // cannot happen for a table the host entry built; workgroup-uniform
    const bool sym = sg.kind < 2;
    int tm, tn;
    if (sym) {                                                // row-major list of the tiles with tn >= tm
        tm = 0;
        while (t >= sg.tcols - tm) { t -= sg.tcols - tm; ++tm; }
        tn = tm + t;
    } else {
        tm = t / sg.tcols;
        tn = t - tm * sg.tcols;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const GtAccLanes at;
    const bool a_is_y = sg.kind == 1, b_is_x = sg.kind == 0;
    GtRowFetch fa, fb;
    fa.bind(a_is_y ? Y : X, a_is_y ? ldy : ldx, a_is_y ? iy : ix, sg.a0, tm * 64, sg.na, tid);
    fb.bind(b_is_x ? X : Y, b_is_x ? ldx : ldy, b_is_x ? ix : iy, sg.b0, tn * 64, sg.nb, tid);
    double4_t acc[2][2];
    gt_acc_zero(acc);
    gemm_tile_64x64_rows_f32(fa, fb, d, acc, lds);

    const bool diag = sym && tm == tn;
    double s = 0.0;
    if constexpr (KF == MMD_POLY3) {
        // epilogue on the accumulator registers: k = (dot / d + 1)^3 (a true division: 1 / d is not exact for d = 100 or 192 and
        // its error would not average out over a sum of positive terms), rows / columns beyond the group and i == j masked
        const double dd = (double)d;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tm * 64 + at.row(a, r), col = tn * 64 + at.col(b);
                    const double v = acc[a][b][r] / dd + 1.0;
                    const bool on = row < sg.na && col < sg.nb && !(diag && row == col);
                    s += on ? v * v * v : 0.0;
                }
    } else {
        // k = exp(-gamma d2) on the accumulator registers, d2 = rows_d2 as in csrc/knn.hip; the same masks.  A row or column past
        // the group reads its last position's norm (the tile fetched that row too) and is masked.
        const double* norm_a = a_is_y ? rbf.ny + (sg.a0 - rbf.y0) : rbf.nx + (sg.a0 - rbf.x0);
        const double* norm_b = b_is_x ? rbf.nx + (sg.b0 - rbf.x0) : rbf.ny + (sg.b0 - rbf.y0);
        double na[2][4];
        gt_rows_load(na, norm_a, tm * 64, sg.na, at);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int col = tn * 64 + at.col(b);
            const double nb = norm_b[col < sg.nb ? col : sg.nb - 1];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = tm * 64 + at.row(a, r);
                    const double d2 = rows_d2(na[a][r], nb, acc[a][b][r]);
                    const bool on = row < sg.na && col < sg.nb && !(diag && row == col);
                    s += on ? exp(-rbf.gamma * d2) : 0.0;
                }
        }
    }
    s = wave_sum(s);
    double* wsum = reinterpret_cast<double*>(lds);            // every wave is past the K loop's last barrier
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (tid == 0) {
        const double w = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        partial[bid] = (sym && tn > tm) ? 2.0 * w : w;
    }
}

__global__ __launch_bounds__(256) void mmd_reduce_kernel(const MmdSeg* __restrict__ segs, const double* __restrict__ partial,
                                                               double* __restrict__ out) {
    __shared__ double sh[256];
    const int tile0 = segs[blockIdx.x].tile0, n = segs[blockIdx.x].ntiles;
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[tile0 + i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];           // segment = 3 * group + kind: the (n_groups, 3) output
}

// ---- host side ---------------------------------------------------------------------------------------------------------
#define MMD_MAX_GROUP_ROWS ((int64_t)1 << 24)

static size_t mmd_table_bytes(int n_groups) { return (((size_t)n_groups * 3 * sizeof(MmdSeg)) + 255) & ~(size_t)255; }

// offsets -> segment table (segs == nullptr: only the tile total).  Every size a kernel loops over or indexes with is fixed here.
static int mmd_plan(const int64_t* ox, const int64_t* oy, int n_groups, std::vector<MmdSeg>* segs, int64_t* total) {
    if (!ox || !oy || n_groups < 0 || !total) return TISE_ERR_INVALID_ARG;
    if (n_groups > (1 << 20)) return TISE_ERR_UNSUPPORTED;
    if (n_groups > 0 && (ox[0] < 0 || oy[0] < 0)) return TISE_ERR_INVALID_ARG;
    int64_t tiles = 0;
    for (int g = 0; g < n_groups; ++g) {
        const int64_t n = ox[g + 1] - ox[g], m = oy[g + 1] - oy[g];
        if (n < 0 || m < 0) return TISE_ERR_INVALID_ARG;
        if (n > MMD_MAX_GROUP_ROWS || m > MMD_MAX_GROUP_ROWS) return TISE_ERR_UNSUPPORTED;
        const int64_t tx = (n + 63) / 64, ty = (m + 63) / 64;
        const int64_t cnt[3] = {tx * (tx + 1) / 2, ty * (ty + 1) / 2, tx * ty};
        for (int k = 0; k < 3; ++k) {
            if (tiles + cnt[k] > (int64_t)0x7fffffff) return TISE_ERR_UNSUPPORTED;
            if (segs) {
                MmdSeg s;
                s.a0 = k == 1 ? oy[g] : ox[g];
                s.b0 = k == 0 ? ox[g] : oy[g];
                s.na = (int)(k == 1 ? m : n);
                s.nb = (int)(k == 0 ? n : m);
                s.tile0 = (int)tiles;
                s.ntiles = (int)cnt[k];
                s.kind = k;
                s.tcols = (int)(k == 0 ? tx : ty);
                s.pad[0] = s.pad[1] = 0;
                segs->push_back(s);
            }
            tiles += cnt[k];
        }
    }
    *total = tiles;
    return TISE_OK;
}

extern "C" {

int tise_mmd_poly3_workspace_bytes(const int64_t* offsets_x_host, const int64_t* offsets_y_host, int n_groups, size_t* bytes) {
    if (!bytes) return TISE_ERR_INVALID_ARG;
    int64_t total = 0;
    const int rc = mmd_plan(offsets_x_host, offsets_y_host, n_groups, nullptr, &total);
    if (rc != TISE_OK) return rc;
    *bytes = mmd_table_bytes(n_groups) + (size_t)total * sizeof(double);
    return TISE_OK;
}

static int mmd_side_check(const float* p, int64_t rows, int64_t ld, const int64_t* index, int64_t n_index, const int64_t* off,
                          int n_groups, int d) {
    if (n_index < 0 || (!p && rows > 0)) return TISE_ERR_INVALID_ARG;
    const int rc = rows_layout_check(p, rows, ld, d);
    if (rc != TISE_OK) return rc;
    const int64_t last = n_groups > 0 ? off[n_groups] : 0;
    if (last > (index ? n_index : rows)) return TISE_ERR_INVALID_ARG;              // a group would reach past the rows / the index
    if (index && last > 0 && rows == 0) return TISE_ERR_INVALID_ARG;               // an index into no rows
    return TISE_OK;
}

// rows of one side that enter some group: positions offsets[0] .. offsets[n_groups] - 1 (mmd_plan has checked the order)
static int64_t mmd_used(const int64_t* off, int n_groups) { return n_groups > 0 ? off[n_groups] - off[0] : 0; }

static int mmd_grouped(int kf, double gamma, const float* x_dev, int64_t rows_x, int64_t ld_x, const int64_t* index_x_dev,
                       int64_t n_index_x, const int64_t* offsets_x_host, const float* y_dev, int64_t rows_y, int64_t ld_y,
                       const int64_t* index_y_dev, int64_t n_index_y, const int64_t* offsets_y_host, int n_groups, int d,
                       double* out_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    if (!rows_width_ok(d) || !out_dev) return TISE_ERR_INVALID_ARG;
    if (kf == MMD_RBF && !(gamma >= 0.0 && gamma <= 1.7976931348623157e308)) return TISE_ERR_INVALID_ARG;   // NaN, inf, < 0
    std::vector<MmdSeg> segs;
    int64_t total = 0;
    int rc = mmd_plan(offsets_x_host, offsets_y_host, n_groups, &segs, &total);
    if (rc != TISE_OK) return rc;
    rc = mmd_side_check(x_dev, rows_x, ld_x, index_x_dev, n_index_x, offsets_x_host, n_groups, d);
    if (rc != TISE_OK) return rc;
    rc = mmd_side_check(y_dev, rows_y, ld_y, index_y_dev, n_index_y, offsets_y_host, n_groups, d);
    if (rc != TISE_OK) return rc;
    if (n_groups == 0) return TISE_OK;
    const size_t table = mmd_table_bytes(n_groups);
    const int64_t cx = kf == MMD_RBF ? mmd_used(offsets_x_host, n_groups) : 0, cy = kf == MMD_RBF ? mmd_used(offsets_y_host, n_groups) : 0;
    const size_t need = table + (size_t)(total + cx + cy) * sizeof(double);
    if (!ws_dev || (reinterpret_cast<uintptr_t>(ws_dev) & 7) || ws_bytes < need) return TISE_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    MmdSeg* segs_dev = reinterpret_cast<MmdSeg*>(ws_dev);
    double* partial = reinterpret_cast<double*>(reinterpret_cast<char*>(ws_dev) + table);
    // the table is built in pageable memory of this call: wait for its copy before the vector goes away
    TISE_HIP_CHECK(hipMemcpyAsync(segs_dev, segs.data(), segs.size() * sizeof(MmdSeg), hipMemcpyHostToDevice, st));
    TISE_HIP_CHECK(hipStreamSynchronize(st));
    const int nseg = 3 * n_groups;
    MmdRbf rbf = {nullptr, nullptr, 0, 0, 0.0};
    if (kf == MMD_RBF) {
        double* norm = partial + total;
        rbf = {norm, norm + cx, offsets_x_host[0], offsets_y_host[0], gamma};
        if (cx + cy > 0) {
            rc = rows_norm2(x_dev, ld_x, index_x_dev, rbf.x0, cx, y_dev, ld_y, index_y_dev, rbf.y0, cy, d, norm, st);
            if (rc != TISE_OK) return rc;
        }
    }
    if (total > 0) {
        if (kf == MMD_RBF)
            hipLaunchKernelGGL(mmd_tiles_kernel<MMD_RBF>, dim3((unsigned)total), dim3(256), 0, st, x_dev, ld_x, index_x_dev, y_dev, ld_y,
                               index_y_dev, d, segs_dev, nseg, partial, rbf);
        else
            hipLaunchKernelGGL(mmd_tiles_kernel<MMD_POLY3>, dim3((unsigned)total), dim3(256), 0, st, x_dev, ld_x, index_x_dev, y_dev, ld_y,
                               index_y_dev, d, segs_dev, nseg, partial, rbf);
        TISE_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(mmd_reduce_kernel, dim3(nseg), dim3(256), 0, st, segs_dev, partial, out_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

int tise_mmd_poly3_grouped(const float* x_dev, int64_t rows_x, int64_t ld_x, const int64_t* index_x_dev, int64_t n_index_x,
                           const int64_t* offsets_x_host, const float* y_dev, int64_t rows_y, int64_t ld_y,
                           const int64_t* index_y_dev, int64_t n_index_y, const int64_t* offsets_y_host, int n_groups, int d,
                           double* out_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    return mmd_grouped(MMD_POLY3, 0.0, x_dev, rows_x, ld_x, index_x_dev, n_index_x, offsets_x_host, y_dev, rows_y, ld_y, index_y_dev,
                       n_index_y, offsets_y_host, n_groups, d, out_dev, ws_dev, ws_bytes, stream);
}

// workspace = the polynomial kernel's + one double per row that enters a group, per side (the squared norms)
int tise_mmd_rbf_workspace_bytes(const int64_t* offsets_x_host, const int64_t* offsets_y_host, int n_groups, size_t* bytes) {
    const int rc = tise_mmd_poly3_workspace_bytes(offsets_x_host, offsets_y_host, n_groups, bytes);
    if (rc != TISE_OK) return rc;
    *bytes += (size_t)(mmd_used(offsets_x_host, n_groups) + mmd_used(offsets_y_host, n_groups)) * sizeof(double);
    return TISE_OK;
}

int tise_mmd_rbf_grouped(const float* x_dev, int64_t rows_x, int64_t ld_x, const int64_t* index_x_dev, int64_t n_index_x,
                         const int64_t* offsets_x_host, const float* y_dev, int64_t rows_y, int64_t ld_y,
                         const int64_t* index_y_dev, int64_t n_index_y, const int64_t* offsets_y_host, int n_groups, int d,
                         double gamma, double* out_dev, void* ws_dev, size_t ws_bytes, void* stream) {
    return mmd_grouped(MMD_RBF, gamma, x_dev, rows_x, ld_x, index_x_dev, n_index_x, offsets_x_host, y_dev, rows_y, ld_y, index_y_dev,
                       n_index_y, offsets_y_host, n_groups, d, out_dev, ws_dev, ws_bytes, stream);
}

}  // extern "C"
