// Hand-written kernels of the CLIP towers (ViT-B/32; the ViT-L/14@336 image tower of CMMD) (text_relevance/RP_coco.py:56-80 and
// positional_alignment/PA.py:33-43 call the third-party `clip` model once per item; here the towers run batched).
// fp16 tensors, fp32 accumulation / statistics, as the fp16 model `clip.load` serves on a GPU computes.
//
//   gemm_f16_kernel      out = act(A W^T + bias) + residual      nn.Linear / the patch-embedding conv / the projections
//   gemm_f16_big_kernel  128 x 128 x 64 tiles, 4 waves (64 x 64 per wave), two workgroups per CU; for launches of many
//                        tiles 256 x 256 x 64, 8 waves (128 x 64 per wave), one workgroup per CU.  Both:
//                        v_mfma_f32_32x32x16_f16, operands global -> LDS by global_load_lds_dwordx4 in 128-BYTE rows
//                        (a K-step of 64 halves is one line), two stages, XOR-swizzled LDS rows (conflict-free
//                        ds_read_b128), epilogue staged per wave so that rows leave as full lines.
//   gemm16_f16_kernel    the same two tile sizes on v_mfma_f32_16x16x32_f16 (the default 128 x 128 instance).
//                        All share gemm_tile (XCD remap -> m0 / n0) and gemm_epilogue (bias, act, rounding, staging, the
//                        full-line store); a kernel body is its DMA, its K-loop and its accumulator map.
//   layernorm_kernel     one wave per row, fp32 mean / variance (CLIP's LayerNorm computes in fp32), eps inside sqrt.
//   attention_f16_kernel one WAVE per (sequence, head): S <= 96 tokens, head dim 64: K Q^T and V^T P^T on the matrix
//                        cores with operands loaded straight into the MFMA layout, fp32 softmax in registers.
//   attention_long_f16_kernel  any S (ViT-L/14@336: 577 tokens), non-causal: 4 waves x 32 queries of one (sequence, head)
//                        share each 64-key K / V tile in LDS; the same two products, online softmax with the exact running
//                        maximum.  A template over the head width: 64, or the 80 of open_clip ViT-H/14.
//   paired_cosine_kernel one wave per row pair, fp64 in a fixed order: CLIPScore's cosine (clip_score.py).
//   vit_tokens_kernel / text_tokens_f16_kernel / patchify_f16_kernel / patchify_pad_f16_kernel (any patch size, rows
//   padded with zeros to the GEMM's K-step) / gather_rows_kernel: token assembly.
// The DINOv2 tower of FD-DINOv2 (dinov2_hip.HipDino) keeps its residual stream in fp32 -- what torch.autocast(fp16) computes:
//   the GEMM kernels' epilogue is a template parameter (EPI_F16 above, EPI_RES32: out32 = res32 + scale * (A W^T + bias), fp32
//   after the accumulator), act 2 (tise_gemm_f16_act only) is the exact (erf) GELU, and layernorm_kernel / vit_tokens_kernel /
//   gather_rows_kernel are templates over their element types: the float instances are the fp32 stream's.
#include <hip/hip_fp16.h>
#include <cstdlib>
#include "common.h"

namespace {

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef float float16_t __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;

__device__ __attribute__((aligned(128))) unsigned char g_clip_zero_page[128];

#define GM_BK 64

typedef float float4_t __attribute__((ext_vector_type(4)));

struct GemmArgs {
    const _Float16* a; long long lda;
    const _Float16* w; long long ldw;
    const _Float16* bias;                            // [N] or null
    const _Float16* res; long long ldr;              // [M][ldr] or null
    _Float16* out; long long ldo;
    int M, N, K, act;                                // act: 0 none, 1 QuickGELU (x * sigmoid(1.702 x)), 2 exact GELU (erf)
    // EPI_RES32 only (tise_gemm_f16_res32): out32 = res32 + scale * (acc + bias), all in fp32
    const float* scale;                              // [N] or null (= 1)
    const float* res32; long long ldr32;             // [M][ldr32]
    float* out32; long long ldo32;                   // may be res32 itself: a lane reads the 16 bytes it then writes
};

// The epilogue of a GEMM kernel is a template parameter: the main loops are the same code.
//   EPI_F16    out = fp16(act(acc + bias)) [+ fp16 residual, a second rounding]: the fp16 stream of the CLIP towers
//   EPI_RES32  out32 = res32 + scale * (acc + bias): nothing after the accumulator is rounded to fp16 -- the fp32 residual
//              stream of the DINOv2 tower (dinov2_hip.HipDino), LayerScale fused
enum { EPI_F16 = 0, EPI_RES32 = 1 };

// nn.GELU() / F.gelu: 0.5 v (1 + erf(v / sqrt 2)) in fp32.  Far below zero erff returns -1 exactly and the sum is 0: the
// result is -0 there, for v = -inf too (0.5 v * 0 would be NaN); +inf stays +inf and NaN stays NaN.
__device__ __forceinline__ float gelu_erf(float v) {
    const float t = 1.0f + erff(v * 0.70710678118654752440f);
    return t == 0.0f ? -0.0f : (0.5f * v) * t;
}

// EPI_RES32, second half: the wave's 32 x 64 fp32 staging rows (pitch 272 bytes: 256 + 16, so that the rows of a 16-byte
// column of writes start 4 banks apart, as the fp16 pitch of 144 does) leave as whole 256-byte rows = two full lines: 16
// lanes per row, four rows per pass.  One fp32 multiply and one fp32 add per element, never contracted into an fma.
constexpr int GM_PITCH32 = 272;
__device__ __forceinline__ void gemm_store_res32(const GemmArgs& p, const unsigned char* st, int lane, int mrow0, int ncol0) {
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
        const int r = pass * 4 + (lane >> 4), ch = lane & 15;
        const int m = mrow0 + r, n = ncol0 + ch * 4;
        float4_t v = *reinterpret_cast<const float4_t*>(st + r * GM_PITCH32 + ch * 16);
        if (m < p.M && n < p.N) {
            const float4_t rr = *reinterpret_cast<const float4_t*>(p.res32 + (long long)m * p.ldr32 + n);
            if (p.scale) {
                const float4_t s = *reinterpret_cast<const float4_t*>(p.scale + n);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = __fmul_rn(s[k], v[k]);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = __fadd_rn(rr[k], v[k]);
            *reinterpret_cast<float4_t*>(p.out32 + (long long)m * p.ldo32 + n) = v;
        }
    }
}

// The tile of a workgroup: blockIdx.x is remapped so that the workgroups one XCD receives (every eighth) are neighbours
// in the tile order, then row-major over the N tiles.
struct GemmTile { int m0, n0; };
__device__ __forceinline__ GemmTile gemm_tile(unsigned bid, unsigned nwg, int N, int BM, int BN) {
    const unsigned q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
    bid = ((xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    const unsigned tiles_n = (unsigned)(N + BN - 1) / BN;
    return {(int)(bid / tiles_n) * BM, (int)(bid % tiles_n) * BN};
}

// The epilogue of every GEMM kernel: one 32 x 64 block of a wave's accumulators goes through the wave's 32 staging rows
// (at the front of the finished operand stages) and leaves as full lines.  The kernel supplies only the map of its MFMA
// shape: frag(g, h) = piece h (of NH) of column group g (of NG): the four accumulator values of this lane at row `row`
// and columns `col` .. col + 3 of the block; col depends on g alone, so one bias fetch serves the NH pieces of a group.
// The bias is added per element inside the act loop: added to a whole piece in front of the act branches it measured
// 1-6 % slower on the tower GEMMs.
//   EPI_F16    fp16(act(acc + bias)) into rows of GM_PITCH16 bytes, then 8 lanes per row, eight rows per pass: 16 bytes
//              per lane [+ the fp16 residual, added in fp32 and rounded a second time]
//   EPI_RES32  acc + bias in fp32 into rows of GM_PITCH32 bytes, then gemm_store_res32
// Nothing beyond M / N is stored.
struct GemmFrag { int row, col; float4_t v; };
constexpr int GM_PITCH16 = 144;
template <int EPI, int NG, int NH, typename Frag>
__device__ __forceinline__ void gemm_epilogue(const GemmArgs& p, unsigned char* lds, int wave, int lane, int mrow0, int ncol0,
                                              Frag frag) {
    unsigned char* st = lds + wave * (32 * (EPI == EPI_RES32 ? GM_PITCH32 : GM_PITCH16));
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const int cl = frag(g, 0).col;
        half4_t bq = {(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
        if (p.bias && ncol0 + cl < p.N) bq = *reinterpret_cast<const half4_t*>(p.bias + ncol0 + cl);
#pragma unroll
        for (int h = 0; h < NH; ++h) {
            const GemmFrag f = frag(g, h);
            if constexpr (EPI == EPI_RES32) {
                float4_t v;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = f.v[k] + (float)bq[k];
                *reinterpret_cast<float4_t*>(st + f.row * GM_PITCH32 + cl * 4) = v;
            } else {
                half4_t hv;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float v = f.v[k] + (float)bq[k];
                    if (p.act == 1) v = v / (1.0f + __expf(-1.702f * v));
                    else if (p.act == 2) v = gelu_erf(v);
                    hv[k] = (_Float16)v;
                }
                *reinterpret_cast<half4_t*>(st + f.row * GM_PITCH16 + cl * 2) = hv;
            }
        }
    }
    if constexpr (EPI == EPI_RES32) {
        gemm_store_res32(p, st, lane, mrow0, ncol0);
    } else {
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int r = pass * 8 + (lane >> 3), ch = lane & 7;
            const int m = mrow0 + r, n = ncol0 + ch * 8;
            half8_t v = *reinterpret_cast<const half8_t*>(st + r * GM_PITCH16 + ch * 16);
            if (m < p.M && n < p.N) {
                if (p.res) {
                    const half8_t rr = *reinterpret_cast<const half8_t*>(p.res + (long long)m * p.ldr + n);
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = (_Float16)((float)v[k] + (float)rr[k]);
                }
                *reinterpret_cast<half8_t*>(p.out + (long long)m * p.ldo + n) = v;
            }
        }
    }
}

// the map of the 32x32x16 shape: accumulator j (32 columns) of a 32-row block holds row lane & 31 and, in registers
// 4 q .. 4 q + 3, columns 8 q + 4 (lane >> 5) ..: eight column groups g = 4 j + q of one piece
__device__ __forceinline__ auto gemm32_frag(const float16_t (&acc)[2], int lane) {
    return [&acc, lane](int g, int) {
        const float16_t& a = acc[g >> 2];
        const int q = 4 * (g & 3);
        return GemmFrag{lane & 31, 8 * g + 4 * (lane >> 5), float4_t{a[q], a[q + 1], a[q + 2], a[q + 3]}};
    };
}

// Operand DMA of the two 32x32x16 kernels (in scope: p, lds, m0, n0, wave, lane, A_BYTES): a wave fetches rows 32 wave .. + 31
// of both operands of a stage as four pieces of 8 rows x 128 B each (lane -> row lane >> 3, 16-byte chunk lane & 7,
// XOR-swizzled).  Rows beyond M / N read the zero page and do not advance.  Macros, not functions: through a function the
// compiler groups the eight loads of a K-step and pads them with s_nop instead of placing the pointer updates between them.
#define GM32_DMA_SETUP                                                                                    \
    const unsigned char* zp = g_clip_zero_page;                                                           \
    const unsigned char* pa[4];                                                                           \
    const unsigned char* pw[4];                                                                           \
    int ia[4], iw[4];                                                                                     \
    _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                        \
        const int r = (4 * wave + g) * 8 + (lane >> 3);                                                   \
        const int c = (lane & 7) ^ ((r >> 1) & 7);                                                        \
        const bool oka = m0 + r < p.M, okw = n0 + r < p.N;                                                \
        pa[g] = oka ? reinterpret_cast<const unsigned char*>(p.a + (long long)(m0 + r) * p.lda + c * 8) : zp;  \
        ia[g] = oka ? 128 : 0;                                                                            \
        pw[g] = okw ? reinterpret_cast<const unsigned char*>(p.w + (long long)(n0 + r) * p.ldw + c * 8) : zp;  \
        iw[g] = okw ? 128 : 0;                                                                            \
    }
// one K-step (128 bytes of every row) into the stage at byte SOFF
#define GM32_DMA_ISSUE(SOFF)                                                                              \
    {                                                                                                     \
        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                    \
            const unsigned char* s_ = pa[g];                                                               \
            __builtin_amdgcn_global_load_lds(s_, (lds_ptr_t)(lds + (SOFF) + (4 * wave + g) * 1024), 16, 0, 0);            \
            pa[g] = s_ + ia[g];                                                                            \
        }                                                                                                  \
        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                    \
            const unsigned char* s_ = pw[g];                                                               \
            __builtin_amdgcn_global_load_lds(s_, (lds_ptr_t)(lds + (SOFF) + A_BYTES + (4 * wave + g) * 1024), 16, 0, 0);  \
            pw[g] = s_ + iw[g];                                                                            \
        }                                                                                                  \
    }

// 128 x 128 x 64 tiles: four waves (2 x 2 of 64 x 64), TWO LDS stages of 32 KB, two workgroups per CU -- the structure of
// the convolution kernel (conv_split.hip).  The first version used 256 x 128 tiles with eight waves and three stages
// (144 KB of LDS: one workgroup per CU), so the DMA latency in front of a tile's first K-step and its epilogue were
// fully exposed, and the towers' GEMMs are short: K = 512 / 768 is 8 / 12 K-steps.  With two workgroups per CU the
// second one computes meanwhile: 5-15 % faster on every tower shape (tools/clip_gemm_probe.py) although a CU now
// moves 64 KB instead of 48 KB of operands per 128 MFMAs.
template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_f16_kernel(const GemmArgs p) {
    constexpr int BM = 128, BN = 128;
    constexpr int A_BYTES = BM * 128, STAGE = A_BYTES + BN * 128;         // 32 KB
    __shared__ __attribute__((aligned(1024))) unsigned char lds[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const auto [m0, n0] = gemm_tile(blockIdx.x, gridDim.x, p.N, BM, BN);
    GM32_DMA_SETUP
    float16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int frow = lane & 31, fsw = (frow >> 1) & 7;
    int fo[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) fo[s] = frow * 128 + (((2 * s + (lane >> 5)) ^ fsw) * 16);
    const unsigned char* fa = lds + (wm * 64) * 128;
    const unsigned char* fb = lds + A_BYTES + (wn * 64) * 128;
// the first K-slice's fragments are requested before the step's DMA is issued (LDS latency under the issue phase)
#define GS_HEAD(SOFF)                                                                                     \
    {                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                    \
            h_a[i] = *reinterpret_cast<const half8_t*>(fa + (SOFF) + i * 32 * 128 + fo[0]);                \
            h_b[i] = *reinterpret_cast<const half8_t*>(fb + (SOFF) + i * 32 * 128 + fo[0]);                \
        }                                                                                                  \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
    }
#define GS_COMPUTE(SOFF)                                                                                  \
    {                                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        half8_t a_[4][2], b_[4][2];                                                                        \
        _Pragma("unroll") for (int s = 0; s < 4; ++s)                                                      \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                \
                if (s == 0) { a_[0][i] = h_a[i]; b_[0][i] = h_b[i]; }                                      \
                else {                                                                                     \
                    a_[s][i] = *reinterpret_cast<const half8_t*>(fa + (SOFF) + i * 32 * 128 + fo[s]);      \
                    b_[s][i] = *reinterpret_cast<const half8_t*>(fb + (SOFF) + i * 32 * 128 + fo[s]);      \
                }                                                                                          \
            }                                                                                              \
        _Pragma("unroll") for (int s = 0; s < 4; ++s)                                                      \
            _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                  \
                _Pragma("unroll") for (int j = 0; j < 2; ++j)                                              \
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b_[s][j], a_[s][i], acc[i][j], 0, 0, 0); \
        /* slice s+1's four reads go out under slice s's four MFMAs */                                     \
        _Pragma("unroll") for (int s = 0; s < 3; ++s) {                                                    \
            __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);                                             \
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                             \
        }                                                                                                  \
        __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);                                                 \
    }
    half8_t h_a[2], h_b[2];
    const int nsteps = p.K / GM_BK;
    GM32_DMA_ISSUE(0)
    int step = 0;
    for (; step + 1 < nsteps; step += 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        GS_HEAD(0)
        GM32_DMA_ISSUE(STAGE)
        GS_COMPUTE(0)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        GS_HEAD(STAGE)
        if (step + 2 < nsteps) GM32_DMA_ISSUE(0)
        GS_COMPUTE(STAGE)
    }
    if (step < nsteps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        GS_HEAD(0)
        GS_COMPUTE(0)
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
        gemm_epilogue<EPI, 8, 1>(p, lds, wave, lane, m0 + wm * 64 + i * 32, n0 + wn * 64, gemm32_frag(acc[i], lane));
}

// 256 x 256 x 64 tiles for the large GEMMs (at least four tiles per CU): eight waves (2 x 4, 128 x 64 per wave), two
// stages of 64 KB, one workgroup per CU.  A CU moves 64 KB of operands per 256 MFMAs here -- 32 B/clk against the
// 64 B/clk of the 128 x 128 kernel and the ~38 B/clk the LDS-DMA path delivers -- and a wave reads 6 fragments per 8
// MFMAs instead of 4 per 4.  The price is one workgroup per CU: the DMA latency in front of a tile's first K-step and
// its epilogue are exposed, so the launcher uses it only where a tile has enough K-steps and the launch enough tiles.
template <int EPI>
__global__ __launch_bounds__(512, 1) void gemm_f16_big_kernel(const GemmArgs p) {
    constexpr int BM = 256, BN = 256;
    constexpr int A_BYTES = BM * 128, STAGE = A_BYTES + BN * 128;         // 64 KB
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 2, wn = wave & 3;                   // 2 x 4 waves of 128 x 64
    const auto [m0, n0] = gemm_tile(blockIdx.x, gridDim.x, p.N, BM, BN);
    GM32_DMA_SETUP
    float16_t acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    const int frow = lane & 31, fsw = (frow >> 1) & 7;
    int fo[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) fo[s] = frow * 128 + (((2 * s + (lane >> 5)) ^ fsw) * 16);
    const unsigned char* fa = lds + (wm * 128) * 128;
    const unsigned char* fb = lds + A_BYTES + (wn * 64) * 128;
// reads of slice s+1 are written before the MFMAs of slice s (six reads per eight MFMAs)
#define GB_READS(S, SOFF, BUF)                                                                            \
    {                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                      \
            a_[BUF][i] = *reinterpret_cast<const half8_t*>(fa + (SOFF) + i * 32 * 128 + fo[S]);            \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                      \
            b_[BUF][j] = *reinterpret_cast<const half8_t*>(fb + (SOFF) + j * 32 * 128 + fo[S]);            \
    }
#define GB_MFMAS(BUF)                                                                                     \
    _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                          \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                      \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(b_[BUF][j], a_[BUF][i], acc[i][j], 0, 0, 0);
#define GB_COMPUTE(SOFF)                                                                                  \
    {                                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        GB_READS(1, SOFF, 1) GB_MFMAS(0) __builtin_amdgcn_sched_barrier(0);                                \
        GB_READS(2, SOFF, 0) GB_MFMAS(1) __builtin_amdgcn_sched_barrier(0);                                \
        GB_READS(3, SOFF, 1) GB_MFMAS(0) __builtin_amdgcn_sched_barrier(0);                                \
        GB_MFMAS(1) __builtin_amdgcn_sched_barrier(0);                                                     \
    }
    half8_t a_[2][4], b_[2][2];
    const int nsteps = p.K / GM_BK;
    GM32_DMA_ISSUE(0)
    int step = 0;
    for (; step + 1 < nsteps; step += 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        GB_READS(0, 0, 0)
        __builtin_amdgcn_sched_barrier(0);
        GM32_DMA_ISSUE(STAGE)
        GB_COMPUTE(0)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        GB_READS(0, STAGE, 0)
        __builtin_amdgcn_sched_barrier(0);
        if (step + 2 < nsteps) GM32_DMA_ISSUE(0)
        GB_COMPUTE(STAGE)
    }
    if (step < nsteps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        GB_READS(0, 0, 0)
        GB_COMPUTE(0)
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
        gemm_epilogue<EPI, 8, 1>(p, lds, wave, lane, m0 + wm * 128 + i * 32, n0 + wn * 64, gemm32_frag(acc[i], lane));
}

#undef GM32_DMA_SETUP
#undef GM32_DMA_ISSUE

// ------------------------------------------------------------------------------------------------
// Round 4: both GEMM kernels on v_mfma_f32_16x16x32_f16 (gemm16_f16_kernel<BIG>).  Same tiles, LDS images, DMA and
// epilogue staging as the two kernels above; inside a wave a fragment is 16 rows x 32 K (lane -> row lane & 15, 16-byte
// chunk lane >> 4 of the K-step's first or second 64 bytes) and the accumulator four-register blocks of 16 x 16.  The
// convolution kernels made the same move in round 3 (same flop, same LDS bytes, but the K = 32 shape reads and
// writes half the accumulator registers per flop and the chip holds 1.79 instead of 1.52 GHz under its power limit).
// The chunk swizzle is the convolution kernels' tise_lds_swz (conflict-free for 16-row fragments).
// BIG = false: 128 x 128 x 64 tiles, 4 waves of 64 x 64, two workgroups per CU;  BIG = true: 256 x 256 x 64, 8 waves of
// 128 x 64, one per CU.  TISE_GEMM_SHAPE=32 selects the 32x32x16 kernels above (A/B of tools/clip_gemm_probe.py).
template <bool BIG, int EPI>
__global__ __launch_bounds__(BIG ? 512 : 256, BIG ? 1 : 2) void gemm16_f16_kernel(const GemmArgs p) {
    constexpr int BM = BIG ? 256 : 128, BN = BM;
    constexpr int NW = BIG ? 8 : 4;
    constexpr int WM = BIG ? 128 : 64;                          // rows of A per wave; 64 columns (rows of W) per wave
    constexpr int MI = WM / 16, NI = 4;                         // 16-row fragments per wave along m and n
    constexpr int A_BYTES = BM * 128, STAGE = A_BYTES + BN * 128;
    extern __shared__ __attribute__((aligned(1024))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = BIG ? (wave >> 2) : (wave >> 1), wn = BIG ? (wave & 3) : (wave & 1);
    const auto [m0, n0] = gemm_tile(blockIdx.x, gridDim.x, p.N, BM, BN);
    // DMA pieces (8 rows x 128 B): this wave fetches rows 32 wave .. +31 of both operands.  Source = one scalar base per
    // operand (advanced by 128 bytes per K-step on the scalar unit) + a constant 32-bit byte offset per lane and piece (the
    // `saddr` form of the instruction: no per-step vector arithmetic, 8 address registers instead of 24).  Rows beyond M
    // (N) are CLAMPED to the last valid row instead of redirected to a zero page: a row of the product depends on its own
    // operand row only, and rows / columns beyond M / N are never stored.
    const unsigned char* abase = reinterpret_cast<const unsigned char*>(p.a + (long long)m0 * p.lda);
    const unsigned char* wbase = reinterpret_cast<const unsigned char*>(p.w + (long long)n0 * p.ldw);
    unsigned offa[4], offw[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int r = (4 * wave + g) * 8 + (lane >> 3);
        const int c = (lane & 7) ^ tise_lds_swz(r);
        const int ra = m0 + r < p.M ? r : p.M - 1 - m0, rw = n0 + r < p.N ? r : p.N - 1 - n0;
        offa[g] = (unsigned)ra * (unsigned)p.lda * 2u + c * 16;
        offw[g] = (unsigned)rw * (unsigned)p.ldw * 2u + c * 16;
    }
#define G16_ISSUE(SOFF)                                                                                   \
    {                                                                                                     \
        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                    \
            const unsigned char* s_ = abase + offa[g];                                                     \
            __builtin_amdgcn_global_load_lds(s_, (lds_ptr_t)(lds + (SOFF) + (4 * wave + g) * 1024), 16, 0, 0);            \
        }                                                                                                  \
        _Pragma("unroll") for (int g = 0; g < 4; ++g) {                                                    \
            const unsigned char* s_ = wbase + offw[g];                                                     \
            __builtin_amdgcn_global_load_lds(s_, (lds_ptr_t)(lds + (SOFF) + A_BYTES + (4 * wave + g) * 1024), 16, 0, 0);  \
        }                                                                                                  \
        abase += 128; wbase += 128;                                                                        \
    }
    float4_t acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = float4_t{0.f, 0.f, 0.f, 0.f};
    // fragment: row (lane & 15) of a 16-row block, chunk (lane >> 4) of K-slice 0 (slice 1: chunk + 4 = address ^ 64)
    const int f16o = (lane & 15) * 128 + (((lane >> 4) ^ tise_lds_swz(lane & 15)) << 4);
    const unsigned char* fa = lds + (wm * WM) * 128;
    const unsigned char* fb = lds + A_BYTES + (wn * 64) * 128;
    half8_t a_[MI], b_[2][NI];
// K-slice 0 of the stage: all fragments
#define G16_READS(SOFF)                                                                                   \
    {                                                                                                     \
        _Pragma("unroll") for (int i = 0; i < MI; ++i)                                                     \
            a_[i] = *reinterpret_cast<const half8_t*>(fa + (SOFF) + i * 2048 + f16o);                      \
        _Pragma("unroll") for (int j = 0; j < NI; ++j)                                                     \
            b_[0][j] = *reinterpret_cast<const half8_t*>(fb + (SOFF) + j * 2048 + f16o);                   \
    }
// slice 0's MFMAs row block by row block; a row block's slice-1 fragment is requested into the registers its slice-0
// fragment has just left (the LDS latency passes under the following blocks' MFMAs; 64 + 32 fragment registers live
// instead of 96 + 48: the 256 x 256 instance would spill otherwise), then slice 1's MFMAs
#define G16_COMPUTE(SOFF)                                                                                 \
    {                                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
        _Pragma("unroll") for (int j = 0; j < NI; ++j)                                                     \
            b_[1][j] = *reinterpret_cast<const half8_t*>(fb + (SOFF) + j * 2048 + (f16o ^ 64));            \
        _Pragma("unroll") for (int i = 0; i < MI; ++i) {                                                   \
            _Pragma("unroll") for (int j = 0; j < NI; ++j)                                                 \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b_[0][j], a_[i], acc[i][j], 0, 0, 0);   \
            a_[i] = *reinterpret_cast<const half8_t*>(fa + (SOFF) + i * 2048 + (f16o ^ 64));               \
            __builtin_amdgcn_sched_barrier(0);                                                             \
        }                                                                                                  \
        _Pragma("unroll") for (int i = 0; i < MI; ++i)                                                     \
            _Pragma("unroll") for (int j = 0; j < NI; ++j)                                                 \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b_[1][j], a_[i], acc[i][j], 0, 0, 0);   \
        __builtin_amdgcn_sched_barrier(0);                                                                 \
    }
    const int nsteps = p.K / GM_BK;
    G16_ISSUE(0)
    int step = 0;
    for (; step + 1 < nsteps; step += 2) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        G16_READS(0)
        __builtin_amdgcn_sched_barrier(0);
        G16_ISSUE(STAGE)
        G16_COMPUTE(0)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        G16_READS(STAGE)
        __builtin_amdgcn_sched_barrier(0);
        if (step + 2 < nsteps) G16_ISSUE(0)
        G16_COMPUTE(STAGE)
    }
    if (step < nsteps) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        G16_READS(0)
        G16_COMPUTE(0)
    }
    __syncthreads();
#undef G16_ISSUE
#undef G16_READS
#undef G16_COMPUTE
    // epilogue: the accumulator block (i, j) holds row m = 16 i + (lane & 15) and the four columns n = 16 j + 4 (lane >> 4) + k
    // of this lane: per 32 rows, four column groups of two pieces
#pragma unroll
    for (int i2 = 0; i2 < MI / 2; ++i2)
        gemm_epilogue<EPI, NI, 2>(p, lds, wave, lane, m0 + wm * WM + i2 * 32, n0 + wn * 64, [&](int j, int h) {
            return GemmFrag{16 * h + (lane & 15), 16 * j + 4 * (lane >> 4), acc[2 * i2 + h][j]};
        });
}

// eight consecutive elements of a row, moved as 16-byte pieces (one of eight halves, two of four floats), read and
// written as fp32
template <typename T> struct Row8;
template <> struct Row8<_Float16> {
    half8_t h = {};
    __device__ void load(const _Float16* src) { h = *reinterpret_cast<const half8_t*>(src); }
    __device__ void store(_Float16* dst) const { *reinterpret_cast<half8_t*>(dst) = h; }
    __device__ float get(int e) const { return (float)h[e]; }
    __device__ void set(int e, float f) { h[e] = (_Float16)f; }
};
template <> struct Row8<float> {
    float4_t q[2] = {};
    __device__ void load(const float* src) {
        q[0] = *reinterpret_cast<const float4_t*>(src);
        q[1] = *reinterpret_cast<const float4_t*>(src + 4);
    }
    __device__ void store(float* dst) const {
        *reinterpret_cast<float4_t*>(dst) = q[0];
        *reinterpret_cast<float4_t*>(dst + 4) = q[1];
    }
    __device__ float get(int e) const { return q[e >> 2][e & 3]; }
    __device__ void set(int e, float f) { q[e >> 2][e & 3] = f; }
};

// one wave per row: y = (x - mean) / sqrt(var + eps) * gamma + beta, statistics in fp32 (two passes over registers).
// 16-byte loads and stores: lane l holds columns 8l .. 8l+7 and 512 + 8l .. (C <= 1024, C % 8 == 0) -- the first
// version moved 2 bytes per lane and instruction and ran at 2 TB/s.
// InT = _Float16 (x, gamma, beta and out in fp16): the CLIP towers, rsqrtf.  InT = float: the fp32 residual stream of the
// DINOv2 tower (dinov2_hip.HipDino), 1 / sqrtf; OutT = _Float16 feeds the next GEMM, float is the tower's feature row.
// NG = 16-byte groups per lane: 2 (C <= 1024) everywhere but tise_layernorm_wide_f16, whose NG = 4 holds a row of up to 2048
// columns (open_clip ViT-H/14: 1280) -- the same loops, 32 sequential adds per lane instead of 16; groups beyond C add +0.
template <typename InT, typename OutT, int NG>
__global__ __launch_bounds__(256) void layernorm_kernel(const InT* __restrict__ x, long long ldx, const InT* __restrict__ gamma,
                                                        const InT* __restrict__ beta, OutT* __restrict__ out, long long ldo,
                                                        int rows, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const InT* xr = x + (long long)row * ldx;
    float v[NG][8];
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int c = 512 * k + 8 * lane;
        Row8<InT> r;
        if (c < C) r.load(xr + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) { v[k][e] = r.get(e); s += v[k][e]; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    const float mean = s / (float)C;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        if (512 * k + 8 * lane < C) {
#pragma unroll
            for (int e = 0; e < 8; ++e) { const float d = v[k][e] - mean; q += d * d; }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off, 64);
    const float rstd = sizeof(InT) == 2 ? rsqrtf(q / (float)C + eps) : 1.0f / sqrtf(q / (float)C + eps);
    OutT* o = out + (long long)row * ldo;
#pragma unroll
    for (int k = 0; k < NG; ++k) {
        const int c = 512 * k + 8 * lane;
        if (c < C) {
            Row8<InT> g, bb;
            g.load(gamma + c);
            bb.load(beta + c);
            Row8<OutT> r;
#pragma unroll
            for (int e = 0; e < 8; ++e) r.set(e, (v[k][e] - mean) * rstd * g.get(e) + bb.get(e));
            r.store(o + c);
        }
    }
}

// qkv: [B*S][3*E] (q | k | v, head h = columns h*64 .. h*64+63 of each), out: [B*S][E].  ONE WAVE per (sequence, head),
// everything on the matrix cores:
//   S^T[j][i] = sum_d K[j][d] Q[i][d]    A operand = K rows, B operand = Q rows: both are 8 consecutive d per lane, i.e.
//                                         16-byte loads straight from global memory into the MFMA operand layout;
//   the accumulator of a lane then holds ONE query i = lane & 31 and keys j = 32 jt + 8 g + 4 (lane >> 5) + k' along
//   its registers: the softmax over the keys is an in-lane reduction plus one exchange with lane ^ 32;
//   O^T[d][i] = sum_j V^T[d][j] P^T[j][i]  B operand = the probabilities exactly as they sit in the registers (fp16);
//                                         A operand = V^T rows from an LDS copy of V transposed on the way in.  The
//   K index of that product is permuted (j runs 4h + k', 8 + 4h + k' inside a 16-slice) consistently on both operands.
// NT = key / query tiles of 32 (2: S <= 64, the image tower's 50; 3: S <= 96, the text tower's 77).
template <int NT>
__global__ __launch_bounds__(256) void attention_f16_kernel(const _Float16* __restrict__ qkv, int S, int H, int BH, int causal,
                                                            _Float16* __restrict__ out) {
    constexpr int SP = 32 * NT, VP = SP + 8;                   // padded key count; V^T pitch in halves (16-byte aligned rows)
    __shared__ __attribute__((aligned(16))) _Float16 vt_all[4][64 * VP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int bh = blockIdx.x * 4 + wave;
    if (bh >= BH) return;
    const int b = bh / H, h = bh - b * H;
    const int E = H * 64;
    const long long ld = 3LL * E;
    const _Float16* qb = qkv + (long long)b * S * ld + h * 64;
    const _Float16* kb = qb + E;
    const _Float16* vb = qb + 2 * E;
    _Float16* vt = vt_all[wave];
    const int r = lane & 31, hh = lane >> 5;
    // ---- V^T into LDS: lane (row j = 8 t + (lane >> 3), 8 d's = lane & 7) ------------------------------------
    for (int j0 = 0; j0 < SP; j0 += 8) {
        const int j = j0 + (lane >> 3), d0 = (lane & 7) * 8;
        half8_t v8 = {0, 0, 0, 0, 0, 0, 0, 0};
        if (j < S) v8 = *reinterpret_cast<const half8_t*>(vb + (long long)j * ld + d0);
#pragma unroll
        for (int e = 0; e < 8; ++e) vt[(d0 + e) * VP + j] = v8[e];
    }
    // K fragments of every key tile (A operand of the score product): rows j = 32 jt + r, d = 16 ks + 8 hh .. +7
    half8_t kf[NT][4];
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) {
        const int j = 32 * jt + r;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            half8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
            kf[jt][ks] = j < S ? *reinterpret_cast<const half8_t*>(kb + (long long)j * ld + 16 * ks + 8 * hh) : z;
        }
    }
    __builtin_amdgcn_s_waitcnt(0);                              // this wave's LDS writes of V^T are done (in-order per wave)
#pragma unroll 1
    for (int it = 0; it < NT; ++it) {
        const int i = 32 * it + r;                             // this lane's query
        if (32 * it >= S) break;
        half8_t qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            half8_t z = {0, 0, 0, 0, 0, 0, 0, 0};
            qf[ks] = i < S ? *reinterpret_cast<const half8_t*>(qb + (long long)i * ld + 16 * ks + 8 * hh) : z;
        }
        float16_t sc[NT];
#pragma unroll
        for (int jt = 0; jt < NT; ++jt) {
#pragma unroll
            for (int e = 0; e < 16; ++e) sc[jt][e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) sc[jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf[jt][ks], qf[ks], sc[jt], 0, 0, 0);
        }
        // scale, mask, softmax over the keys of query i (registers of this lane and of lane ^ 32)
        float m = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int j = 32 * jt + 8 * (e >> 2) + 4 * hh + (e & 3);
                const bool ok = j < S && !(causal && j > i);
                const float v = ok ? sc[jt][e] * 0.125f : -INFINITY;
                sc[jt][e] = v;
                m = fmaxf(m, v);
            }
        m = fmaxf(m, __shfl_xor(m, 32, 64));
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float pe = (sc[jt][e] == -INFINITY) ? 0.f : __expf(sc[jt][e] - m);
                sc[jt][e] = pe;
                sum += pe;
            }
        sum += __shfl_xor(sum, 32, 64);
        const float inv = sum > 0.f ? 1.0f / sum : 0.f;        // (padding queries i >= S: all masked)
        // P^T as B operand: K-slice (jt, q) = registers 8 q .. 8 q + 7 of tile jt  (j = 32 jt + 16 q + {4 hh + k', 8 + 4 hh + k'})
        float16_t oc[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) oc[dt][e] = 0.f;
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                half8_t pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = (_Float16)(sc[jt][8 * q + e] * inv);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    // V^T rows d = 32 dt + r, the same 8 keys: two runs of four consecutive j
                    const _Float16* vr = vt + (32 * dt + r) * VP + 32 * jt + 16 * q + 4 * hh;
                    const half4_t lo4 = *reinterpret_cast<const half4_t*>(vr);
                    const half4_t hi4 = *reinterpret_cast<const half4_t*>(vr + 8);
                    half8_t vf;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { vf[e] = lo4[e]; vf[4 + e] = hi4[e]; }
                    oc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oc[dt], 0, 0, 0);
                }
            }
        // O^T[d][i]: this lane's query i, d = 32 dt + 8 g + 4 hh + k'
        if (i < S) {
            _Float16* orow = out + ((long long)b * S + i) * E + h * 64;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    half4_t o4;
#pragma unroll
                    for (int k2 = 0; k2 < 4; ++k2) o4[k2] = (_Float16)oc[dt][4 * g + k2];
                    *reinterpret_cast<half4_t*>(orow + 32 * dt + 8 * g + 4 * hh) = o4;
                }
        }
    }
}

// Long sequences (the image tower of ViT-L/14@336: 577 tokens): the same two products as attention_f16_kernel -- S^T = K Q^T
// with one query per lane, P fed from the accumulator registers as the B operand of O^T = V^T P^T with the K index permuted
// alike on both operands -- but the keys STREAM in tiles of ATTN_LONG_KT under an online softmax, so no register holds more
// than one tile of scores and the key loop has no length limit.
//   workgroup = 4 waves = 4 x 32 consecutive queries of ONE (sequence, head); grid = ceil(S / 128) x batch * heads;
//   a K / V tile is staged ONCE per workgroup in LDS and read by all four waves (a quarter of the global traffic of one
//   wave per head): K as [key][64 d] rows of 128 bytes with the GEMM kernels' chunk swizzle, V transposed on the way in
//   ([d][key], two keys packed per 4-byte write).  Two LDS stages: tile t + 1 is fetched into registers before tile t's
//   MFMAs and written after them, ONE barrier per tile.
//   online softmax with the exact running maximum: m' = max(m, tile max), alpha = exp(m - m'), O *= alpha, l = l alpha +
//   sum p, p = exp(s - m') <= 1 BEFORE its fp16 rounding; the tile's P is exponentiated after m' is known, O and l are
//   scaled once per tile.  l is kept as this lane's partial sum (alpha is common to lane and lane ^ 32) and the halves are
//   added once at the end.  Tile 0 holds key 0, so m is finite from the first tile on (alpha = exp(-inf) = 0 there, on
//   O = l = 0).
//   padded keys j >= S: score -inf before the maximum, K and V rows written to LDS as ZEROS (p = 0 times stale bits that
//   read as NaN would be NaN).  Padding queries i >= S compute on q = 0 and store nothing.  EVERY wave -- also one whose 32
//   queries all lie beyond S -- runs every staging step and every barrier: there is no early return and no break.
#define ATTN_LONG_KT 64
// D = head width: 64 (every OpenAI tower) or 80 (open_clip ViT-H/14: width 1280, 16 heads).  The D = 64 instance is the kernel
// as it was -- the same MFMA order, `* 0.125f`, the same online-softmax steps, the same LDS image.  What D = 80 changes:
//   K Q^T      five K-steps of 16 (80 = 5 x 16: no padding on that side); the scores are multiplied in fp32 by the float nearest
//              1 / sqrt(80).
//   V^T P^T    three 32-row output tiles; V^T rows 80 .. 95 are written as ZEROS once, before the first barrier, in both stages
//              (the staging never touches them again), and output columns >= 80 are never stored.
//   K in LDS   [key][80 d] rows of 160 bytes = ten 16-byte chunks; logical chunk c of row r sits at chunk c ^ ((r >> 4) & 1).
//              Why that is conflict-free: a fragment read is one ds_read_b128 in which lane l reads row r = l & 31, chunk
//              2 ks + (l >> 5); the instruction is served in four groups of 16 lanes, rows {0-3, 12-15, 20-27} and
//              {4-11, 16-19, 28-31} of each half-wave, one logical chunk per group, and a group is conflict-free when its 16
//              rows fall into 16 distinct 16-byte slots of the 256-byte bank row.  The slot of (r, c) is (10 r + c') mod 16 and
//              10 r mod 16 = 2 (5 r mod 8) takes the eight EVEN values, by r mod 8; both row sets hold every residue mod 8
//              exactly twice, as {r, r + 24} or {r, r + 8}: two rows that differ in bit 4.  c' = c ^ bit 4 moves one row of each
//              pair to the neighbouring odd slot (c ^ 1 stays inside 0 .. 9): 8 even + 8 odd slots, 16 distinct.  (The XOR
//              with (r >> 1) & 7 of the 128-byte rows needs eight chunks per row.)
//   staging    item q = tid + 256 n: K chunk q % 10 of row q / 10, n = 0 .. 2 (640 chunks, the third pass half idle); V chunk
//              q % 10 of the key PAIR q / 10, n = 0 .. 1 (320 pairs of chunks).  At D = 64 the same map is row tid >> 3 (+ 32),
//              chunk tid & 7, as before.  Two stages, one barrier per tile, no early return.
template <int D>
__global__ __launch_bounds__(256) void attention_long_f16_kernel(const _Float16* __restrict__ qkv, int S, int H, int QB,
                                                                 _Float16* __restrict__ out) {
    static_assert(D == 64 || D == 80, "the head widths that have an LDS layout");
    constexpr int KT = ATTN_LONG_KT, NJ = KT / 32;
    constexpr int NKS = D / 16, NDT = (D + 31) / 32, CH = D / 8; // K-steps of K Q^T; 32-row tiles of V^T P^T; 16-byte chunks per row
    constexpr int KP = 2 * D;                                   // K pitch in bytes
    constexpr int VP = KT + 4;                                  // V^T pitch in halves: 8-byte aligned rows, 34 banks apart
    constexpr int K_BYTES = KT * KP, V_BYTES = 32 * NDT * VP * 2, STAGE = K_BYTES + V_BYTES;
    constexpr int K_ITEMS = KT * CH, V_ITEMS = KT / 2 * CH;     // staging items of a tile and the passes of 256 threads over them
    constexpr int NKP = (K_ITEMS + 255) / 256, NVP = (V_ITEMS + 255) / 256;
    constexpr float SCALE = D == 64 ? 0.125f : 0.111803398874989485f;       // 1 / sqrt(D): exact, or the float nearest 1 / sqrt(80)
    __shared__ __attribute__((aligned(16))) unsigned char lds[2 * STAGE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qb = (int)(blockIdx.x % (unsigned)QB), bh = (int)(blockIdx.x / (unsigned)QB);
    const int b = bh / H, h = bh - b * H;
    const int E = H * D;
    const long long ld = 3LL * E;
    const _Float16* qbase = qkv + (long long)b * S * ld + h * D;
    const _Float16* kb = qbase + E;
    const _Float16* vb = qbase + 2 * E;
    const int r = lane & 31, hh = lane >> 5;
    const int i = qb * 128 + wave * 32 + r;                    // this lane's query
    const half8_t z8 = {0, 0, 0, 0, 0, 0, 0, 0};
    half8_t qf[NKS];
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) qf[ks] = i < S ? *reinterpret_cast<const half8_t*>(qbase + (long long)i * ld + 16 * ks + 8 * hh) : z8;
    // staging: pass n of a thread -> 16-byte chunk kc[n] of K row kr[n]; chunk vc[n] of V rows 2 vq[n], 2 vq[n] + 1
    int kr[NKP], kc[NKP], vq[NVP], vc[NVP];
#pragma unroll
    for (int n = 0; n < NKP; ++n) { kr[n] = (tid + 256 * n) / CH; kc[n] = (tid + 256 * n) % CH; }
#pragma unroll
    for (int n = 0; n < NVP; ++n) { vq[n] = (tid + 256 * n) / CH; vc[n] = (tid + 256 * n) % CH; }
    // a pass beyond the items (D = 80: the upper half of the last one) fetches and writes nothing
    const auto k_on = [&](int n) { return K_ITEMS % 256 == 0 || tid + 256 * n < K_ITEMS; };
    const auto v_on = [&](int n) { return V_ITEMS % 256 == 0 || tid + 256 * n < V_ITEMS; };
    // chunk c of K row `row` in LDS (the comment above)
    const auto k_swz = [](int c, int row) { return D == 64 ? c ^ ((row >> 1) & 7) : c ^ ((row >> 4) & 1); };
    half8_t gk[NKP], gv[NVP][2];
#define AL_FETCH(J0)                                                                                       \
    {                                                                                                     \
        _Pragma("unroll") for (int n = 0; n < NKP; ++n) {                                                  \
            const int jk = (J0) + kr[n];                                                                   \
            gk[n] = (k_on(n) && jk < S) ? *reinterpret_cast<const half8_t*>(kb + (long long)jk * ld + 8 * kc[n]) : z8; \
        }                                                                                                  \
        _Pragma("unroll") for (int n = 0; n < NVP; ++n)                                                    \
            _Pragma("unroll") for (int u = 0; u < 2; ++u) {                                                \
                const int jv = (J0) + 2 * vq[n] + u;                                                       \
                gv[n][u] = (v_on(n) && jv < S) ? *reinterpret_cast<const half8_t*>(vb + (long long)jv * ld + 8 * vc[n]) : z8; \
            }                                                                                              \
    }
#define AL_WRITE(SOFF)                                                                                     \
    {                                                                                                     \
        _Pragma("unroll") for (int n = 0; n < NKP; ++n)                                                    \
            if (k_on(n)) *reinterpret_cast<half8_t*>(lds + (SOFF) + kr[n] * KP + (k_swz(kc[n], kr[n]) << 4)) = gk[n]; \
        _Float16* vt_ = reinterpret_cast<_Float16*>(lds + (SOFF) + K_BYTES);                               \
        _Pragma("unroll") for (int n = 0; n < NVP; ++n)                                                    \
            if (v_on(n)) {                                                                                 \
                _Pragma("unroll") for (int e = 0; e < 8; ++e) {                                            \
                    half2_t pr = {gv[n][0][e], gv[n][1][e]};                                               \
                    *reinterpret_cast<half2_t*>(vt_ + (8 * vc[n] + e) * VP + 2 * vq[n]) = pr;               \
                }                                                                                          \
            }                                                                                              \
    }
    float16_t oc[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) oc[dt][e] = 0.f;
    float m = -INFINITY, l = 0.f;
    const int T = (S + KT - 1) / KT;                            // the same for every wave of the workgroup
    if constexpr (32 * NDT > D) {                               // V^T rows D .. 32 NDT - 1 of both stages: zeros, written once
        constexpr int ZW = (32 * NDT - D) * VP / 2;             // dwords; the rows are contiguous
        for (int w = tid; w < 2 * ZW; w += 256)
            *reinterpret_cast<unsigned*>(lds + (w / ZW) * STAGE + K_BYTES + D * VP * 2 + (w % ZW) * 4) = 0u;
    }
    AL_FETCH(0)
    AL_WRITE(0)
    __syncthreads();
    const int ksw = D == 64 ? (r >> 1) & 7 : (r >> 4) & 1;
#pragma unroll 1
    for (int t = 0; t < T; ++t) {
        const int soff = (t & 1) * STAGE;
        const int j0 = t * KT;
        if (t + 1 < T) AL_FETCH(j0 + KT)                       // uniform over the workgroup
        const unsigned char* kl = lds + soff;
        const _Float16* vt = reinterpret_cast<const _Float16*>(lds + soff + K_BYTES);
        float16_t s[NJ];
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[jt][e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const half8_t kf = *reinterpret_cast<const half8_t*>(kl + (32 * jt + r) * KP + (((2 * ks + hh) ^ ksw) << 4));
                s[jt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[ks], s[jt], 0, 0, 0);
            }
        }
        // scale, mask the padded keys, tile maximum of query i (this lane's registers and lane ^ 32's)
        float tm = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int j = j0 + 32 * jt + 8 * (e >> 2) + 4 * hh + (e & 3);
                const float v = j < S ? s[jt][e] * SCALE : -INFINITY;
                s[jt][e] = v;
                tm = fmaxf(tm, v);
            }
        tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
        const float mn = fmaxf(m, tm);                         // finite: tile 0 holds key 0
        const float alpha = __expf(m - mn);                    // tile 0: exp(-inf) = 0 on O = l = 0
        m = mn;
        float psum = 0.f;
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float pe = __expf(s[jt][e] - mn);        // exp(-inf) = 0 for the padded keys
                s[jt][e] = pe;
                psum += pe;
            }
        l = l * alpha + psum;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int e = 0; e < 16; ++e) oc[dt][e] *= alpha;
#pragma unroll
        for (int jt = 0; jt < NJ; ++jt)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                half8_t pf;
#pragma unroll
                for (int e = 0; e < 8; ++e) pf[e] = (_Float16)s[jt][8 * q + e];
#pragma unroll
                for (int dt = 0; dt < NDT; ++dt) {
                    const _Float16* vr = vt + (32 * dt + r) * VP + 32 * jt + 16 * q + 4 * hh;
                    const half4_t lo4 = *reinterpret_cast<const half4_t*>(vr);
                    const half4_t hi4 = *reinterpret_cast<const half4_t*>(vr + 8);
                    half8_t vf;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { vf[e] = lo4[e]; vf[4 + e] = hi4[e]; }
                    oc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf, oc[dt], 0, 0, 0);
                }
            }
        if (t + 1 < T) AL_WRITE(STAGE - soff)                  // the stage tile t - 1 was read from: every wave passed the barrier since
        __syncthreads();
    }
#undef AL_FETCH
#undef AL_WRITE
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;                                 // l >= 1: the key of the maximum contributes exp(0)
    if (i < S) {
        _Float16* orow = out + ((long long)b * S + i) * E + h * D;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (32 * dt + 8 * g >= D) continue;             // D = 80: rows 80 .. 95 of the third tile are padding, never stored
                half4_t o4;
#pragma unroll
                for (int k2 = 0; k2 < 4; ++k2) o4[k2] = (_Float16)(oc[dt][4 * g + k2] * inv);
                *reinterpret_cast<half4_t*>(orow + 32 * dt + 8 * g + 4 * hh) = o4;
            }
    }
}

// image (B, 3, R, R) fp16 NCHW -> patch matrix [B * (R/P)^2][3 * P * P], column = c * P*P + ky * P + kx (= the
// flattening of conv1.weight (width, 3, P, P)), so that the patch embedding is one GEMM
__global__ __launch_bounds__(256) void patchify_f16_kernel(const _Float16* __restrict__ img, int B, int R, int P,
                                                           _Float16* __restrict__ out) {
    const int G = R / P, K = 3 * P * P;
    const long long total = (long long)B * G * G * K / 8;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const long long el = e * 8;
        const int col = (int)(el % K);
        const long long row = el / K;
        const int c = col / (P * P), ky = (col / P) % P, kx = col % P;          // kx multiple of 8
        const int b = (int)(row / (G * G)), gy = (int)(row / G % G), gx = (int)(row % G);
        const _Float16* src = img + (((long long)b * 3 + c) * R + gy * P + ky) * R + gx * P + kx;
        *reinterpret_cast<half8_t*>(out + el) = *reinterpret_cast<const half8_t*>(src);
    }
}

// the same patch matrix for ANY patch size, rows padded to KP >= 3 P^2 columns (KP % 64 == 0: tise_gemm_f16's K-step): one
// output element per thread, 2-byte reads, stores consecutive along the output row; columns 3 P^2 .. KP - 1 are written as +0
__global__ __launch_bounds__(256) void patchify_pad_f16_kernel(const _Float16* __restrict__ img, int B, int R, int P, int KP,
                                                               _Float16* __restrict__ out) {
    const int G = R / P, K = 3 * P * P;
    const long long total = (long long)B * G * G * KP;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int col = (int)(e % KP);
        const long long row = e / KP;
        _Float16 v = (_Float16)0.f;
        if (col < K) {
            const int c = col / (P * P), ky = (col / P) % P, kx = col % P;
            const int b = (int)(row / (G * G)), gy = (int)(row / G % G), gx = (int)(row % G);
            v = img[(((long long)b * 3 + c) * R + gy * P + ky) * R + gx * P + kx];
        }
        out[e] = v;
    }
}

// x[b][0] = class_emb + pos[0];  x[b][1 + p] = patch_out[b * NP + p] + pos[1 + p]          (width W)
// patch_out is the fp16 output of the patch GEMM; class row, position table and tokens are T: _Float16 in the CLIP towers,
// float in the fp32 stream of the DINOv2 tower.  One fp32 add per element.
template <typename T>
__global__ __launch_bounds__(256) void vit_tokens_kernel(const _Float16* __restrict__ patch_out, const T* __restrict__ cls,
                                                         const T* __restrict__ pos, int B, int NP, int W, T* __restrict__ x) {
    const long long total = (long long)B * (NP + 1) * W;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % W);
        const long long t = e / W;
        const int s = (int)(t % (NP + 1));
        const long long b = t / (NP + 1);
        const float base = s == 0 ? (float)cls[c] : (float)patch_out[(b * NP + s - 1) * W + c];
        x[e] = (T)(base + (float)pos[(long long)s * W + c]);
    }
}

// x[b][s] = table[tokens[b][s]] + pos[s]
__global__ __launch_bounds__(256) void text_tokens_f16_kernel(const int* __restrict__ tokens, const _Float16* __restrict__ table,
                                                              const _Float16* __restrict__ pos, long long rows, int S, int W,
                                                              _Float16* __restrict__ x) {
    const long long total = rows * W;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % W);
        const long long t = e / W;
        const int s = (int)(t % S);
        x[e] = (_Float16)((float)table[(long long)tokens[t] * W + c] + (float)pos[(long long)s * W + c]);
    }
}

// out[i] = x[index[i]]  (rows of width W; the class token of every image / the end-of-text token of every caption)
template <typename T>
__global__ __launch_bounds__(256) void gather_rows_kernel(const T* __restrict__ x, const long long* __restrict__ index, long long n,
                                                          int W, T* __restrict__ out) {
    const long long total = n * W;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int c = (int)(e % W);
        const long long i = e / W;
        out[e] = x[index[i] * W + c];
    }
}

// CLIPScore's paired cosine: out[i] = (a_i . b_i) / sqrt((a_i . a_i)(b_i . b_i)) of row i of two (n, d) tables, ONE WAVE per row.
// Every product and sum is fp64 (a product of two fp16 or fp32 values is exact there) in a fixed order: lane l adds the
// elements l, l + 64, ... in turn, then a butterfly (xor 32 .. 1) leaves the same total in every lane.  No atomics: two launches
// give the same bits.  A zero row is 0 / sqrt(0) = NaN, as numpy's 0 / 0.  Not a hot path (n * d reads once).
template <typename T>
__global__ __launch_bounds__(256) void paired_cosine_kernel(const T* __restrict__ a, const T* __restrict__ b, long long n, int d,
                                                            double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const T* ar = a + row * d;
    const T* br = b + row * d;
    double ab = 0.0, aa = 0.0, bb = 0.0;
    for (int c = lane; c < d; c += 64) {
        const double x = (double)ar[c], y = (double)br[c];
        ab += x * y;
        aa += x * x;
        bb += y * y;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        ab += __shfl_xor(ab, off, 64);
        aa += __shfl_xor(aa, off, 64);
        bb += __shfl_xor(bb, off, 64);
    }
    if (lane == 0) out[row] = ab / sqrt(aa * bb);
}

inline int grid1d(long long total) {
    long long b = (total + 255) / 256;
    return (int)(b > 16384 ? 16384 : (b < 1 ? 1 : b));
}

// the instance rule and the launch, the same for every epilogue (p.M > 0)
template <int EPI>
int gemm_launch(const GemmArgs& p, void* stream) {
    const int m = p.M, n = p.N;
    const long long tiles = (long long)((m + 127) / 128) * ((n + 127) / 128);
    if (tiles > 0x7fffffffLL) return TISE_ERR_UNSUPPORTED;
    // TISE_GEMM_BIG: 0 never, 1 (default) by the rule below, 2 always -- the A/B switch of tools/clip_gemm_probe.py
    static const int big_mode = [] { const char* e = getenv("TISE_GEMM_BIG"); return e ? atoi(e) : 1; }();
    const long long tiles_big = (long long)((m + 255) / 256) * ((n + 255) / 256);
    // TISE_GEMM_SHAPE: 16 = the v_mfma_f32_16x16x32_f16 kernels for every launch, 32 = round 2's 32x32x16 kernels for every
    // launch, unset = by measurement (tools/clip_gemm_probe.py, profiles/r04b_clip_gemm_shapes.txt): the 128 x 128 kernel
    // is 12-14 % faster on the K = 32 shape (660 -> 754, 889 -> 1001, 877 -> 984 TFLOP/s), the 256 x 256 kernel 8-14 %
    // SLOWER (its 128 x 64 wave tile needs the slice-1 fragments re-loaded row block by row block to stay inside 256
    // registers, which serialises its issue stream), so it stays on 32x32x16
    static const int shape = [] { const char* e = getenv("TISE_GEMM_SHAPE"); return e ? atoi(e) : 0; }();
    // act 2 stays on the 128 x 128 kernel under the default rule: erff is some 40 VALU instructions per element, which a
    // second workgroup on the CU hides under its MFMAs and the one-per-CU kernel cannot (DINOv2 ViT-L/14 fc1, 12 850 x 4096 x
    // 1024: 209 us on the 256 x 256 kernel; the whole tower 14.88 -> 14.12 ms, profiles/r15a_dinov2_probe.txt)
    const bool big = big_mode == 2 || (big_mode == 1 && tiles_big >= 768 && p.act != 2);
    if (shape == 16 || (shape == 0 && !big)) {
        constexpr int lds_big = 2 * (256 * 128 + 256 * 128), lds_small = 2 * (128 * 128 + 128 * 128);
        static std::atomic<unsigned long long> attr16{0};
        if (tise_first_use_on_this_device(attr16)) {
            TISE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm16_f16_kernel<true, EPI>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds_big));
            TISE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm16_f16_kernel<false, EPI>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds_small));
        }
        if (big) hipLaunchKernelGGL((gemm16_f16_kernel<true, EPI>), dim3((unsigned)tiles_big), dim3(512), lds_big, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((gemm16_f16_kernel<false, EPI>), dim3((unsigned)tiles), dim3(256), lds_small, (hipStream_t)stream, p);
        TISE_LAUNCH_CHECK();
        return TISE_OK;
    }
    if (big) {
        constexpr int lds_big = 2 * (256 * 128 + 256 * 128);
        static std::atomic<unsigned long long> attr_set{0};
        if (tise_first_use_on_this_device(attr_set))
            TISE_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(gemm_f16_big_kernel<EPI>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, lds_big));
        hipLaunchKernelGGL(gemm_f16_big_kernel<EPI>, dim3((unsigned)tiles_big), dim3(512), lds_big, (hipStream_t)stream, p);
        TISE_LAUNCH_CHECK();
        return TISE_OK;
    }
    hipLaunchKernelGGL(gemm_f16_kernel<EPI>, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, p);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

// What every GEMM entry point asks of a / w / bias and the shape, and their half of the arguments: the kernels move a / w
// rows by 16-byte LDS-DMA and bias in 8-byte pieces, so strides below the row length and misaligned pointers are refused
// (false) before anything reaches the device.
bool gemm_operands(GemmArgs& p, const void* a_dev, int64_t lda, const void* w_dev, int64_t ldw, const void* bias_dev, int m, int n, int k) {
    if (!a_dev || !w_dev || m < 0 || n <= 0 || k <= 0 || k % GM_BK != 0 || n % 8 != 0 || lda % 8 != 0 || ldw % 8 != 0 || lda < k ||
        ldw < k || ((reinterpret_cast<uintptr_t>(a_dev) | reinterpret_cast<uintptr_t>(w_dev)) & 15) != 0 ||
        (reinterpret_cast<uintptr_t>(bias_dev) & 7) != 0)
        return false;
    p.a = reinterpret_cast<const _Float16*>(a_dev); p.lda = lda;
    p.w = reinterpret_cast<const _Float16*>(w_dev); p.ldw = ldw;
    p.bias = reinterpret_cast<const _Float16*>(bias_dev);
    p.M = m; p.N = n; p.K = k;
    return true;
}

// tise_gemm_f16 (act 0 .. 1, as it always was) and tise_gemm_f16_act (act 0 .. 2): one check, one launch
int gemm_f16_entry(const void* a_dev, int64_t lda, const void* w_dev, int64_t ldw, const void* bias_dev, const void* res_dev,
                   int64_t ldr, void* out_dev, int64_t ldo, int m, int n, int k, int act, int max_act, void* stream) {
    // res / out move in 16-byte pieces of eight halves
    GemmArgs p = {};
    if (!gemm_operands(p, a_dev, lda, w_dev, ldw, bias_dev, m, n, k) || !out_dev || ldo % 8 != 0 || (res_dev && ldr % 8 != 0) ||
        act < 0 || act > max_act || ldo < n || (res_dev && ldr < n) ||
        ((reinterpret_cast<uintptr_t>(out_dev) | reinterpret_cast<uintptr_t>(res_dev)) & 15) != 0)
        return TISE_ERR_INVALID_ARG;
    if (m == 0) return TISE_OK;
    p.res = reinterpret_cast<const _Float16*>(res_dev); p.ldr = ldr;
    p.out = reinterpret_cast<_Float16*>(out_dev); p.ldo = ldo;
    p.act = act;
    return gemm_launch<EPI_F16>(p, stream);
}

// tise_layernorm_f16, tise_layernorm_wide_f16 (NG = 4) and both outputs of tise_layernorm_f32: x, gamma, beta and out move as
// 16-byte pieces of eight halves or four floats; C <= 512 NG
template <typename InT, typename OutT, int NG = 2>
int layernorm_launch(const void* x_dev, int64_t ldx, const void* gamma_dev, const void* beta_dev, void* out_dev, int64_t ldo,
                     int64_t rows, int C, float eps, void* stream) {
    constexpr int64_t xmul = 16 / sizeof(InT), omul = 16 / sizeof(OutT);
    if (!x_dev || !gamma_dev || !beta_dev || !out_dev || rows < 0 || C <= 0 || C > 512 * NG || C % 8 != 0 || ldx % xmul != 0 ||
        ldo % omul != 0 || ldx < C || ldo < C ||
        ((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(out_dev) | reinterpret_cast<uintptr_t>(gamma_dev) |
          reinterpret_cast<uintptr_t>(beta_dev)) & 15) != 0)
        return TISE_ERR_INVALID_ARG;
    if (rows == 0) return TISE_OK;
    if ((rows + 3) / 4 > 0x7fffffffLL) return TISE_ERR_UNSUPPORTED;
    hipLaunchKernelGGL((layernorm_kernel<InT, OutT, NG>), dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const InT*>(x_dev), ldx, reinterpret_cast<const InT*>(gamma_dev),
                       reinterpret_cast<const InT*>(beta_dev), reinterpret_cast<OutT*>(out_dev), ldo, (int)rows, C, eps);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

template <typename T>
int vit_tokens_launch(const void* patch_out_dev, const void* class_dev, const void* pos_emb_dev, int batch, int n_patches, int width,
                      void* x_dev, void* stream) {
    if (!patch_out_dev || !class_dev || !pos_emb_dev || !x_dev || batch < 0 || n_patches <= 0 || width <= 0) return TISE_ERR_INVALID_ARG;
    if (batch == 0) return TISE_OK;
    hipLaunchKernelGGL(vit_tokens_kernel<T>, dim3(grid1d((long long)batch * (n_patches + 1) * width)), dim3(256), 0,
                       (hipStream_t)stream, reinterpret_cast<const _Float16*>(patch_out_dev), reinterpret_cast<const T*>(class_dev),
                       reinterpret_cast<const T*>(pos_emb_dev), batch, n_patches, width, reinterpret_cast<T*>(x_dev));
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

template <typename T>
int gather_rows_launch(const void* x_dev, const int64_t* index_dev, int64_t n, int width, void* out_dev, void* stream) {
    if (!x_dev || !index_dev || !out_dev || n < 0 || width <= 0) return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    hipLaunchKernelGGL(gather_rows_kernel<T>, dim3(grid1d(n * width)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const T*>(x_dev), reinterpret_cast<const long long*>(index_dev), (long long)n, width,
                       reinterpret_cast<T*>(out_dev));
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

}  // namespace

extern "C" {

int tise_gemm_f16(const void* a_dev, int64_t lda, const void* w_dev, int64_t ldw, const void* bias_dev, const void* res_dev,
                  int64_t ldr, void* out_dev, int64_t ldo, int m, int n, int k, int act, void* stream) {
    return gemm_f16_entry(a_dev, lda, w_dev, ldw, bias_dev, res_dev, ldr, out_dev, ldo, m, n, k, act, 1, stream);
}

int tise_gemm_f16_act(const void* a_dev, int64_t lda, const void* w_dev, int64_t ldw, const void* bias_dev, const void* res_dev,
                      int64_t ldr, void* out_dev, int64_t ldo, int m, int n, int k, int act, void* stream) {
    return gemm_f16_entry(a_dev, lda, w_dev, ldw, bias_dev, res_dev, ldr, out_dev, ldo, m, n, k, act, 2, stream);
}

int tise_gemm_f16_res32(const void* a_dev, int64_t lda, const void* w_dev, int64_t ldw, const void* bias_dev, const void* scale_dev,
                        const void* res32_dev, int64_t ldr, void* out32_dev, int64_t ldo, int m, int n, int k, void* stream) {
    // res32 / out32 move in 16-byte pieces of four floats (rows 16-byte aligned: strides % 4), scale in 16-byte pieces.
    // out32 == res32 (same stride) is the tower's in-place update; any other overlap is the caller's.
    GemmArgs p = {};
    if (!gemm_operands(p, a_dev, lda, w_dev, ldw, bias_dev, m, n, k) || !res32_dev || !out32_dev || ldr % 4 != 0 || ldo % 4 != 0 ||
        ldr < n || ldo < n ||
        ((reinterpret_cast<uintptr_t>(res32_dev) | reinterpret_cast<uintptr_t>(out32_dev) | reinterpret_cast<uintptr_t>(scale_dev)) & 15) != 0)
        return TISE_ERR_INVALID_ARG;
    if (m == 0) return TISE_OK;
    p.scale = reinterpret_cast<const float*>(scale_dev);
    p.res32 = reinterpret_cast<const float*>(res32_dev); p.ldr32 = ldr;
    p.out32 = reinterpret_cast<float*>(out32_dev); p.ldo32 = ldo;
    return gemm_launch<EPI_RES32>(p, stream);
}

int tise_layernorm_f32(const void* x_dev, int64_t ldx, const void* gamma_dev, const void* beta_dev, void* out_dev, int64_t ldo,
                       int64_t rows, int C, float eps, int out_f32, void* stream) {
    if (out_f32 != 0 && out_f32 != 1) return TISE_ERR_INVALID_ARG;
    return out_f32 ? layernorm_launch<float, float>(x_dev, ldx, gamma_dev, beta_dev, out_dev, ldo, rows, C, eps, stream)
                   : layernorm_launch<float, _Float16>(x_dev, ldx, gamma_dev, beta_dev, out_dev, ldo, rows, C, eps, stream);
}

int tise_vit_tokens_f32(const void* patch_out_dev, const void* class_tok_dev, const void* pos_emb_dev, int batch, int n_patches,
                        int width, void* x_dev, void* stream) {
    if ((reinterpret_cast<uintptr_t>(patch_out_dev) & 1) != 0 ||
        ((reinterpret_cast<uintptr_t>(class_tok_dev) | reinterpret_cast<uintptr_t>(pos_emb_dev) | reinterpret_cast<uintptr_t>(x_dev)) & 3) != 0)
        return TISE_ERR_INVALID_ARG;
    return vit_tokens_launch<float>(patch_out_dev, class_tok_dev, pos_emb_dev, batch, n_patches, width, x_dev, stream);
}

int tise_gather_rows_f32(const void* x_dev, const int64_t* index_dev, int64_t n, int width, void* out_dev, void* stream) {
    if (((reinterpret_cast<uintptr_t>(x_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 3) != 0 ||
        (reinterpret_cast<uintptr_t>(index_dev) & 7) != 0)
        return TISE_ERR_INVALID_ARG;
    return gather_rows_launch<float>(x_dev, index_dev, n, width, out_dev, stream);
}

int tise_layernorm_f16(const void* x_dev, int64_t ldx, const void* gamma_dev, const void* beta_dev, void* out_dev, int64_t ldo,
                       int64_t rows, int C, float eps, void* stream) {
    return layernorm_launch<_Float16, _Float16>(x_dev, ldx, gamma_dev, beta_dev, out_dev, ldo, rows, C, eps, stream);
}

int tise_layernorm_wide_f16(const void* x_dev, int64_t ldx, const void* gamma_dev, const void* beta_dev, void* out_dev, int64_t ldo,
                            int64_t rows, int C, float eps, void* stream) {
    return layernorm_launch<_Float16, _Float16, 4>(x_dev, ldx, gamma_dev, beta_dev, out_dev, ldo, rows, C, eps, stream);
}

int tise_paired_cosine(const void* img_dev, const void* txt_dev, int64_t n, int d, int is_f16, double* out_cos_dev, void* stream) {
    const uintptr_t mask = is_f16 ? 1 : 3;
    if (!img_dev || !txt_dev || !out_cos_dev || n < 0 || d <= 0 || (is_f16 != 0 && is_f16 != 1) ||
        ((reinterpret_cast<uintptr_t>(img_dev) | reinterpret_cast<uintptr_t>(txt_dev)) & mask) != 0 ||
        (reinterpret_cast<uintptr_t>(out_cos_dev) & 7) != 0)
        return TISE_ERR_INVALID_ARG;
    if (n == 0) return TISE_OK;
    if ((n + 3) / 4 > 0x7fffffffLL) return TISE_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((n + 3) / 4)), block(256);
    if (is_f16)
        hipLaunchKernelGGL(paired_cosine_kernel<_Float16>, grid, block, 0, (hipStream_t)stream, reinterpret_cast<const _Float16*>(img_dev),
                           reinterpret_cast<const _Float16*>(txt_dev), (long long)n, d, out_cos_dev);
    else
        hipLaunchKernelGGL(paired_cosine_kernel<float>, grid, block, 0, (hipStream_t)stream, reinterpret_cast<const float*>(img_dev),
                           reinterpret_cast<const float*>(txt_dev), (long long)n, d, out_cos_dev);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

int tise_attention_f16(const void* qkv_dev, int batch, int seq, int heads, int head_dim, int causal, void* out_dev, void* stream) {
    if (!qkv_dev || !out_dev || batch < 0 || seq <= 0 || seq > 96 || heads <= 0 || head_dim != 64 ||
        ((reinterpret_cast<uintptr_t>(qkv_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15) != 0)    // 16-byte q / k / v loads
        return TISE_ERR_INVALID_ARG;
    if (batch == 0) return TISE_OK;
    const long long bh = (long long)batch * heads;
    if ((bh + 3) / 4 > 0x7fffffffLL) return TISE_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)((bh + 3) / 4)), block(256);
    const _Float16* q = reinterpret_cast<const _Float16*>(qkv_dev);
    _Float16* o = reinterpret_cast<_Float16*>(out_dev);
    if (seq <= 32) hipLaunchKernelGGL(attention_f16_kernel<1>, grid, block, 0, (hipStream_t)stream, q, seq, heads, (int)bh, causal, o);
    else if (seq <= 64) hipLaunchKernelGGL(attention_f16_kernel<2>, grid, block, 0, (hipStream_t)stream, q, seq, heads, (int)bh, causal, o);
    else hipLaunchKernelGGL(attention_f16_kernel<3>, grid, block, 0, (hipStream_t)stream, q, seq, heads, (int)bh, causal, o);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

int tise_attention_long_key_tile(void) { return ATTN_LONG_KT; }

int tise_attention_long_f16(const void* qkv_dev, int batch, int seq, int heads, int head_dim, void* out_dev, void* stream) {
    // 16-byte q / k / v loads: the q, k and v base of every head is 16-byte aligned when qkv is (a head is 128 or 160 bytes)
    if (!qkv_dev || !out_dev || batch < 0 || seq <= 0 || heads <= 0 || (head_dim != 64 && head_dim != 80) ||
        ((reinterpret_cast<uintptr_t>(qkv_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15) != 0)
        return TISE_ERR_INVALID_ARG;
    if (batch == 0) return TISE_OK;
    const long long qblocks = ((long long)seq + 127) / 128;
    const long long bh = (long long)batch * heads;
    if (qblocks * bh > 0x7fffffffLL) return TISE_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(qblocks * bh)), block(256);
    const _Float16* q = reinterpret_cast<const _Float16*>(qkv_dev);
    _Float16* o = reinterpret_cast<_Float16*>(out_dev);
    if (head_dim == 64) hipLaunchKernelGGL(attention_long_f16_kernel<64>, grid, block, 0, (hipStream_t)stream, q, seq, heads, (int)qblocks, o);
    else hipLaunchKernelGGL(attention_long_f16_kernel<80>, grid, block, 0, (hipStream_t)stream, q, seq, heads, (int)qblocks, o);
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

int tise_patchify_f16(const void* img_dev, int batch, int res, int patch, void* out_dev, void* stream) {
    if (!img_dev || !out_dev || batch < 0 || res <= 0 || patch <= 0 || res % patch != 0 || patch % 8 != 0 ||
        ((reinterpret_cast<uintptr_t>(img_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 15) != 0)    // 16-byte loads / stores
        return TISE_ERR_INVALID_ARG;
    if (batch == 0) return TISE_OK;
    const long long total = (long long)batch * (res / patch) * (res / patch) * 3 * patch * patch / 8;
    hipLaunchKernelGGL(patchify_f16_kernel, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const _Float16*>(img_dev), batch, res, patch, reinterpret_cast<_Float16*>(out_dev));
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

int tise_patchify_pad_f16(const void* img_dev, int batch, int res, int patch, int kpad, void* out_dev, void* stream) {
    if (!img_dev || !out_dev || batch < 0 || res <= 0 || patch <= 0 || res % patch != 0 || kpad <= 0 || kpad % 64 != 0 ||
        3LL * patch * patch > kpad || (reinterpret_cast<uintptr_t>(img_dev) & 1) != 0 || (reinterpret_cast<uintptr_t>(out_dev) & 15) != 0)
        return TISE_ERR_INVALID_ARG;
    if (batch == 0) return TISE_OK;
    const long long total = (long long)batch * (res / patch) * (res / patch) * kpad;
    hipLaunchKernelGGL(patchify_pad_f16_kernel, dim3(grid1d(total)), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const _Float16*>(img_dev), batch, res, patch, kpad, reinterpret_cast<_Float16*>(out_dev));
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

int tise_vit_tokens_f16(const void* patch_out_dev, const void* class_emb_dev, const void* pos_emb_dev, int batch, int n_patches,
                        int width, void* x_dev, void* stream) {
    return vit_tokens_launch<_Float16>(patch_out_dev, class_emb_dev, pos_emb_dev, batch, n_patches, width, x_dev, stream);
}

int tise_text_tokens_f16(const int32_t* tokens_dev, const void* table_dev, const void* pos_emb_dev, int64_t rows, int seq, int width,
                         void* x_dev, void* stream) {
    if (!tokens_dev || !table_dev || !pos_emb_dev || !x_dev || rows < 0 || seq <= 0 || width <= 0) return TISE_ERR_INVALID_ARG;
    if (rows == 0) return TISE_OK;
    hipLaunchKernelGGL(text_tokens_f16_kernel, dim3(grid1d(rows * width)), dim3(256), 0, (hipStream_t)stream, tokens_dev,
                       reinterpret_cast<const _Float16*>(table_dev), reinterpret_cast<const _Float16*>(pos_emb_dev), (long long)rows, seq,
                       width, reinterpret_cast<_Float16*>(x_dev));
    TISE_LAUNCH_CHECK();
    return TISE_OK;
}

int tise_gather_rows_f16(const void* x_dev, const int64_t* index_dev, int64_t n, int width, void* out_dev, void* stream) {
    return gather_rows_launch<_Float16>(x_dev, index_dev, n, width, out_dev, stream);
}

}  // extern "C"
