// IS* temperature calibration: mean NLL, its derivative in T and the ECE bins of temperature-scaled logits, one pass.
//
// Replaces, per evaluation at temperature T, the reference's nn.CrossEntropyLoss()(logits / T, labels) with its
// backward in T (classifier_calibration/temperature_scaling.py:41,64-67) and _ECELoss (:80-119) on cached logits.
// The LBFGS loop itself stays on the host (calibration.py); every loss / gradient it asks for is one call here.
//
// Per row (z = fp32 logits z[c0 .. c0+C), y = label), in fp64 unless stated:
//   m   = max z                    (fp32, exact), pred = FIRST index that attains it
//   d_c = z_c - m                  (exact in fp64 for the fp32 logits of a network: exponents within 29 of each other)
//   e_c = exp(d_c * inv_t)         inv_t = fl(1 / T); the product is one rounding, ocml exp <= 1 ulp
//   s   = sum e_c,  sd = sum d_c e_c                (lane-strided partial sums, then a fixed xor butterfly)
//   nll = log s - (z_y - m) * inv_t                 = -log softmax(z / T)_y
//   g   = ((z_y - m) - sd / s) * inv_t * inv_t      = d nll / dT  = (z_y - sum_c p_c z_c) / T^2
//   conf = fl32(1 / s)             max softmax: the argmax term is exp(0) = 1; rounded to fp32 before binning, as the
//                                  reference bins its fp32 softmax
//   bin  = b with edges[b] < conf <= edges[b+1]    edges = the caller's fp32 torch.linspace(0, 1, n_bins + 1)
// A row whose C logits are not all finite, or whose label is outside [0, C), enters no sum: it is counted in out[2] /
// out[3] instead.  The label selects z_y among the values already loaded (no indexed read: a bad label cannot read
// out of bounds).
//
// Domain: T with a finite 1 / T (T > 2^-1024 = 5.56e-309; for a smaller, subnormal T inv_t is +inf and the maximum's own term would
// be exp(0 * inf) = NaN) and T <= 2^100; anything else is refused on the host before a launch.  The upper limit is what
// the register forms' padding relies on: a padded column holds -FLT_MAX and contributes exp((-FLT_MAX - m) / T), which
// is exactly 0 only while (FLT_MAX + m) / T stays above ~745.  With a row maximum m >= -2^127 and T <= 2^100 the
// argument is <= -(2^27 - 16), far below that.  A row whose maximum lies below -2^127 is outside the documented input
// (the fp32 logits of a network); the streaming form has no padding and no such limit.
//
// Output (4 + 3 n_bins doubles): [sum nll, sum g, rows with a non-finite logit, rows with a bad label,
//                                 count[b], sum conf[b], sum correct[b]  (b < n_bins)]
// The counts are exact (integers below 2^53); the sums are fp64 in a fixed order.
//
// Row-to-wave mapping: the kernel is HBM-bound (4 C bytes per row, read once), so what matters is the bytes each wave
// has in flight when it issues its loads.  A group of G lanes takes one row and every lane keeps K = 16 (32) values of
// it in registers: G = 64 for C in (256, 1024] (2048 with K = 32) and G = 16 / 8 / 4 for C <= 256 / 128 / 64, so a wave
// loads 64 / G rows at once and has up to 4 KB (8 KB) in flight at every C; one wave per row would leave 200 B in
// flight per wave at C = 50.  Rows wider than 2048 are read twice (max, then the sums: the second read mostly hits L2).
//
// Determinism: every block walks a fixed set of rows (grid = f(rows, C) only), each lane sums in row order, waves
// reduce with the fixed butterfly of wave_sum, a block folds its four waves in order into its column of the workspace,
// and calib_fold_kernel sums those columns in block order.  No atomics: bitwise reproducible.
#include <cfloat>
#include <cmath>
#include "common.h"

namespace {

#define CALIB_WAVES 4
#define CALIB_MAX_BLOCKS 2048
#define CALIB_MAX_BINS 64
#define CALIB_MAX_TEMPERATURE 0x1p100              // largest T accepted (see "Domain" above)

struct RowTerms {
    double nll, g;
    float conf;
    int pred, bad;
};

// in-group butterflies (groups of G lanes are aligned, so xor offsets < G stay inside the group)
template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int G>
__device__ __forceinline__ float group_sum_f(float v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <int G>
__device__ __forceinline__ void group_argmax(float& m, int& am) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
        const float om = __shfl_xor(m, off, 64);
        const int oa = __shfl_xor(am, off, 64);
        if (om > m || (om == m && oa < am)) { m = om; am = oa; }
    }
}

template <int G>
__device__ __forceinline__ int group_or(int v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v |= __shfl_xor(v, off, 64);
    return v;
}

// loss terms from the group's max / label value / sums (identical in every lane of the group)
__device__ __forceinline__ void finish_row(float m, float zy, double s, double sd, double inv_t, RowTerms& t) {
    const double dy = (double)zy - (double)m;
    t.nll = log(s) - dy * inv_t;
    t.g = (dy - sd / s) * inv_t * inv_t;
    t.conf = (float)(1.0 / s);
}

// one row held in registers: K values per lane, lane j of the group holds columns j, j + G, j + 2G, ...
// Columns past C hold -FLT_MAX (finite, never loaded): below every real maximum or tied with it at a higher column, so
// never the argmax; in the sums exp(d / T) underflows to exactly 0 (for T <= 2^100 and m >= -2^127: "Domain" in the
// header) and d * 0 = -0, so they add nothing -- the loops run
// without a branch per value (measured: the predicated form was VALU-issue bound at 115 us for 50 000 x 1000).
template <int G, int K>
__device__ __forceinline__ void row_terms_reg(const float* __restrict__ z, int C, int y, double inv_t, int gl,
                                              RowTerms& t) {
    float v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = gl + k * G;
        v[k] = c < C ? z[c] : -FLT_MAX;
    }
    float m = -INFINITY, zy = 0.0f;
    int am = 0x7fffffff, bad = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = gl + k * G;
        bad |= (c < C) & !isfinite(v[k]);
        const bool gt = v[k] > m;                    // columns ascend within a lane: the first maximum stays
        m = gt ? v[k] : m;
        am = gt ? c : am;
        zy = c == y ? v[k] : zy;
    }
    group_argmax<G>(m, am);
    bad = group_or<G>(bad);
    zy = group_sum_f<G>(zy);                         // one lane holds z_y, the others 0: exact
    const double mm = (double)m;
    double s = 0.0, sd = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double d = (double)v[k] - mm;
        const double e = exp(d * inv_t);
        s += e;
        sd += d * e;
    }
    s = group_sum<G>(s);
    sd = group_sum<G>(sd);
    finish_row(m, zy, s, sd, inv_t, t);
    t.pred = am;
    t.bad = bad;
}

// rows wider than 64 x 32: one wave per row, read twice
__device__ __forceinline__ void row_terms_stream(const float* __restrict__ z, int C, int y, double inv_t, int lane,
                                                 RowTerms& t) {
    float m = -INFINITY, zy = 0.0f;
    int am = 0x7fffffff, bad = 0;
    for (int c = lane; c < C; c += 64) {
        const float x = z[c];
        bad |= !isfinite(x);
        if (x > m) { m = x; am = c; }
        if (c == y) zy = x;
    }
    group_argmax<64>(m, am);
    bad = group_or<64>(bad);
    zy = group_sum_f<64>(zy);
    const double mm = (double)m;
    double s = 0.0, sd = 0.0;
    for (int c = lane; c < C; c += 64) {
        const double d = (double)z[c] - mm;
        const double e = exp(d * inv_t);
        s += e;
        sd += d * e;
    }
    s = group_sum<64>(s);
    sd = group_sum<64>(sd);
    finish_row(m, zy, s, sd, inv_t, t);
    t.pred = am;
    t.bad = bad;
}

// b with edges[b] < conf <= edges[b + 1], or -1 (edges ascending, nb + 1 of them)
__device__ __forceinline__ int find_bin(float conf, const float* edges, int nb) {
    int lo = 0, hi = nb - 1;                        // smallest b in [0, nb) with conf <= edges[b + 1]
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (conf <= edges[mid + 1]) hi = mid; else lo = mid + 1;
    }
    return (conf > edges[lo] && conf <= edges[lo + 1]) ? lo : -1;
}

// G lanes per row, K values per lane (K = 0: the streaming form, G = 64).  Block: 4 waves; wave w of block b takes
// row groups (b * 4 + w) + i * gridDim.x * 4, each of 64 / G consecutive rows.  Workspace column j of block b:
// ws[j * nblk + b], j < 4 + 3 nb.
template <int G, int K>
__global__ __launch_bounds__(256) void calib_rows_kernel(const float* __restrict__ logits, int64_t rows, int64_t ld,
                                                         int c0, int C, const int* __restrict__ labels, double inv_t,
                                                         const float* __restrict__ edges_dev, int nb,
                                                         double* __restrict__ ws) {
    constexpr int R = 64 / G;
    __shared__ float edges[CALIB_MAX_BINS + 1];
    __shared__ double red[CALIB_WAVES][4 + 3 * CALIB_MAX_BINS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int gl = lane & (G - 1), r = lane / G;
    for (int i = threadIdx.x; i <= nb; i += blockDim.x) edges[i] = edges_dev[i];
    __syncthreads();

    double nll_acc = 0.0, g_acc = 0.0;              // group leaders: their rows, in order
    int n_nonfinite = 0, n_badlabel = 0;
    int b_cnt = 0, b_cor = 0;                       // lane b < nb: bin b of this wave's rows, in order
    double b_conf = 0.0;
    const int64_t stride = (int64_t)gridDim.x * CALIB_WAVES * R;
    for (int64_t base = ((int64_t)blockIdx.x * CALIB_WAVES + w) * R; base < rows; base += stride) {   // wave-uniform
        const int64_t row = base + r;
        const bool live = row < rows;
        const int y = live ? labels[row] : -1;
        const bool label_ok = y >= 0 && y < C;
        const float* z = logits + (live ? row * ld + c0 : 0);
        RowTerms t;
        if constexpr (K > 0) row_terms_reg<G, K>(z, live ? C : 0, y, inv_t, gl, t);
        else row_terms_stream(z, live ? C : 0, y, inv_t, lane, t);
        const bool use = live && label_ok && !t.bad;
        int bin = -1, correct = 0;
        if (use) {
            bin = find_bin(t.conf, edges, nb);
            correct = t.pred == y;
            if (gl == 0) { nll_acc += t.nll; g_acc += t.g; }
        }
        if (gl == 0 && live) { n_nonfinite += t.bad; n_badlabel += !label_ok; }
        // the wave's R rows into the lanes that own their bins, in row order
#pragma unroll
        for (int q = 0; q < R; ++q) {
            const int qb = __builtin_amdgcn_readlane(bin, q * G);
            const float qc = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t.conf), q * G));
            const int qk = __builtin_amdgcn_readlane(correct, q * G);
            if (lane == qb) { b_cnt += 1; b_conf += (double)qc; b_cor += qk; }
        }
    }
    nll_acc = wave_sum(nll_acc);
    g_acc = wave_sum(g_acc);
    const double nf = wave_sum((double)n_nonfinite), bl = wave_sum((double)n_badlabel);
    if (lane == 0) { red[w][0] = nll_acc; red[w][1] = g_acc; red[w][2] = nf; red[w][3] = bl; }
    if (lane < nb) {
        red[w][4 + lane] = (double)b_cnt;
        red[w][4 + nb + lane] = b_conf;
        red[w][4 + 2 * nb + lane] = (double)b_cor;
    }
    __syncthreads();
    const int P = 4 + 3 * nb;
    for (int j = threadIdx.x; j < P; j += blockDim.x)
        ws[(int64_t)j * gridDim.x + blockIdx.x] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
}

// block j: out[j] = sum over the nblk blocks of column j, thread t taking blocks t, t + 256, ... then a fixed tree
__global__ __launch_bounds__(256) void calib_fold_kernel(const double* __restrict__ ws, int nblk, double* __restrict__ out) {
    __shared__ double part[4];
    const double* col = ws + (int64_t)blockIdx.x * nblk;
    double v = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 256) v += col[k];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// lanes per row (G) and values per lane (K; 0 = streaming) for C columns
static inline void calib_shape(int C, int* G, int* K) {
    if (C <= 64) { *G = 4; *K = 16; }
    else if (C <= 128) { *G = 8; *K = 16; }
    else if (C <= 256) { *G = 16; *K = 16; }
    else if (C <= 1024) { *G = 64; *K = 16; }
    else if (C <= 2048) { *G = 64; *K = 32; }
    else { *G = 64; *K = 0; }
}

static inline int calib_blocks(int64_t rows, int C) {
    int G, K;
    calib_shape(C, &G, &K);
    const int64_t rows_per_block = (int64_t)CALIB_WAVES * (64 / G);
    const int64_t n = ceil_div64(rows, rows_per_block);
    return (int)(n < CALIB_MAX_BLOCKS ? n : CALIB_MAX_BLOCKS);
}

}  // namespace

extern "C" {

int tise_calib_workspace_bytes(int64_t rows, int C, int n_bins, size_t* bytes) {
    if (!bytes || rows < 0 || C < 1 || n_bins < 1 || n_bins > CALIB_MAX_BINS) return TISE_ERR_INVALID_ARG;
    *bytes = (size_t)calib_blocks(rows, C) * (size_t)(4 + 3 * n_bins) * sizeof(double);
    return TISE_OK;
}

int tise_calib_eval(const float* logits_dev, int64_t rows, int64_t ld, int c0, int C, const int32_t* labels_dev,
                    double temperature, const float* edges_dev, int n_bins, double* out_dev, void* ws_dev,
                    size_t ws_bytes, void* stream) {
    if (!logits_dev || !labels_dev || !edges_dev || !out_dev || rows < 0 || C < 1 || c0 < 0 ||
        ld < (int64_t)c0 + C || n_bins < 1 || n_bins > CALIB_MAX_BINS || !(temperature > 0.0) ||
        !std::isfinite(temperature))
        return TISE_ERR_INVALID_ARG;
    // the domain the arithmetic supports (header): 1 / T finite, so the maximum's own term is exp(0 * inv_t) = 1 and not
    // exp(0 * inf) = NaN; T <= 2^100, so the register forms' -FLT_MAX padding still underflows to exactly 0
    if (!std::isfinite(1.0 / temperature) || temperature > CALIB_MAX_TEMPERATURE) return TISE_ERR_INVALID_ARG;
    const int nblk = calib_blocks(rows, C);
    const int P = 4 + 3 * n_bins;
    if (nblk > 0 && (!ws_dev || ws_bytes < (size_t)nblk * P * sizeof(double))) return TISE_ERR_INVALID_ARG;
    hipStream_t st = (hipStream_t)stream;
    double* ws = (double*)ws_dev;
    const double inv_t = 1.0 / temperature;
    if (nblk > 0) {
        int G, K;
        calib_shape(C, &G, &K);
#define CALIB_LAUNCH(GG, KK)                                                                                         \
    hipLaunchKernelGGL((calib_rows_kernel<GG, KK>), dim3(nblk), dim3(64 * CALIB_WAVES), 0, st, logits_dev, rows, ld, \
                       c0, C, (const int*)labels_dev, inv_t, edges_dev, n_bins, ws)
        if (G == 4) CALIB_LAUNCH(4, 16);
        else if (G == 8) CALIB_LAUNCH(8, 16);
        else if (G == 16) CALIB_LAUNCH(16, 16);
        else if (K == 16) CALIB_LAUNCH(64, 16);
        else if (K == 32) CALIB_LAUNCH(64, 32);
        else CALIB_LAUNCH(64, 0);
#undef CALIB_LAUNCH
        TISE_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(calib_fold_kernel, dim3(P), dim3(256), 0, st, ws, nblk, out_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

}  // extern "C"
