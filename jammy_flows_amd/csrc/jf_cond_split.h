// Shared by the split-bf16 conditional-block kernels (cond_split_kernels.hip: log-prob and sampling direction; cond_bwd_kernels.hip: the
// adjoint): chunk geometry of the packed W2 image, the reductions over the four coordinate lanes of a row, the supported layer options.
#pragma once
#include "jf_cond_in.h"
#include "jf_cond_regs.h"
#include "jf_mfma.h"

namespace jf {

constexpr int CS_TILES = 9;                        // 16-column MFMA tiles per layer (36 slots x 4 coordinates)
static_assert(CS_SLOTS == 4 * CS_TILES, "one register per slot, four registers per tile");
constexpr int CS_CT = 3;                           // tiles per chunk
constexpr int CS_CPL = CS_TILES / CS_CT;           // chunks per layer
constexpr int CS_KSTEPS = 4;                       // 128 hidden units = 4 x 32
constexpr int CS_NP = 3;                           // bf16 pieces per f32 operand
constexpr int CS_FRAG = 1024;                      // bytes of one A fragment (64 lanes x 8 bf16)
constexpr int CS_W_BYTES = CS_CT * CS_KSTEPS * CS_NP * CS_FRAG;       // 36864
constexpr int CS_B_BYTES = CS_CT * 16 * 4;                            // 192: the chunk's bias, permuted column order
constexpr int CS_CHUNK_BYTES = CS_W_BYTES + CS_B_BYTES;               // 37056 (16-byte multiple)
// second arithmetic (JF_SPLIT_F16X2): every operand = TWO f16 pieces (11 + 11 significant bits), three products (lo hi, hi lo, hi hi) instead of
// six, two fragments per (tile, k-step) instead of three.  Representation error <= 2^-22 per operand -- below the rounding of the f32
// accumulation either arithmetic ends in (scripts/probe/f16split.py: rms error of the 128-term products 2.4e-8 vs 6.8e-8 for a plain f32 matrix
// product, 1.8e-9 for the bf16 triple).  Range: W2 is scaled by a power of two so that its largest entry sits in [2^14, 2^15), h (in (-1, 1)) by
// 2^14, so a low piece leaves the normal f16 range only below 2^-28 of the largest weight / 2^-28 absolute in h -- whether the matrix core
// keeps or flushes such subnormals is then immaterial (<= 4e-9 |w| per term).  The chunk's bias tail carries the bias in scaled units (the
// accumulators start from it) and the inverse scale 2^-(e + 14) that brings the result back (exact).
constexpr int CS_NP16 = 2;
constexpr int CS_W16_BYTES = CS_CT * CS_KSTEPS * CS_NP16 * CS_FRAG;  // 24576
constexpr int CS_B16_BYTES = CS_B_BYTES + 16;                         // bias + {2^-(e + 14), pad}
constexpr int CS_CHUNK16_BYTES = CS_W16_BYTES + CS_B16_BYTES;         // 24784 (16-byte multiple)
constexpr float CS_H_SCALE = 16384.0f;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using f32x2 = __attribute__((ext_vector_type(2))) float;
// power-of-two scale of W2 for the f16 pieces: the largest entry lands in [2^14, 2^15) (exponent clamped: a matrix whose largest entry is
// below 2^-46 or above 2^74 keeps its pieces inside the f16 range only partly -- not a weight matrix)
__device__ __forceinline__ int cs_w_exponent(float wmax) {
    if (!(wmax > 0.f && wmax < INFINITY)) return 0;
    const int e = 14 - ilogbf(wmax);
    return e < -60 ? -60 : (e > 60 ? 60 : e);
}
// largest |W[n][k]| of an (N, H) matrix with row stride ws -> out[0] (out[1..3] = 0): ONE workgroup of 1024 threads walks the matrix (70 K
// elements for the C3 block: ~4 us).  The first version used one atomicMax per wave of a 274-block grid on a zeroed word: 14 us of
// serialised atomics per pack, and a memset node that broke HIP-graph capture on ROCm 7.2.
static __global__ void __launch_bounds__(1024) cs_absmax_kernel(const float* __restrict__ W, int64_t ws, int N, int H, float* __restrict__ out) {
    __shared__ float part[16];
    float m = 0.f;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (H == 128 && ws % 4 == 0 && (reinterpret_cast<uintptr_t>(W) & 15u) == 0) {
        // 16-byte loads: half a wave covers a row, a wave takes 8 rows per turn (4 independent loads in flight), 16 waves 128 rows
        const int half = lane >> 5, l4 = (lane & 31) * 4;
        for (int n0 = 8 * wave; n0 < N; n0 += 128) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int n = n0 + 2 * u + half;
                v[u] = n < N ? *reinterpret_cast<const f32x4*>(W + (int64_t)n * ws + l4) : f32x4{0.f, 0.f, 0.f, 0.f};
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) m = fmaxf(fmaxf(m, fmaxf(fabsf(v[u][0]), fabsf(v[u][1]))), fmaxf(fabsf(v[u][2]), fabsf(v[u][3])));
        }
    } else {
        for (int n0 = 4 * wave; n0 < N; n0 += 64) {                // a wave takes 4 rows per turn: independent loads, no index division
            for (int k = lane; k < H; k += 64) {
                float v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = n0 + u < N ? W[(int64_t)(n0 + u) * ws + k] : 0.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) m = fmaxf(m, fabsf(v[u]));
            }
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x < 4) {
        float t = 0.f;
        if (threadIdx.x == 0) {
#pragma unroll
            for (int w = 0; w < 16; ++w) t = fmaxf(t, part[w]);
        }
        out[threadIdx.x] = t;
    }
}
template <int NP> struct CsGeom;
template <> struct CsGeom<3> { static constexpr int W = CS_W_BYTES, B = CS_B_BYTES, CHUNK = CS_CHUNK_BYTES; };
template <> struct CsGeom<2> { static constexpr int W = CS_W16_BYTES, B = CS_B16_BYTES, CHUNK = CS_CHUNK16_BYTES; };
// v (two values) -> packed f16 pairs {hi0, hi1} and {lo0, lo1}: hi = RN_f16(v), lo = RN_f16(v - hi)
__device__ __forceinline__ void cs_split16(float v0, float v1, unsigned& hi, unsigned& lo) {
    const f16x2 h = __builtin_convertvector(f32x2{v0, v1}, f16x2);
    const f32x2 back = __builtin_convertvector(h, f32x2);
    const f16x2 l = __builtin_convertvector(f32x2{v0 - back[0], v1 - back[1]}, f16x2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
// the same values for operands that are NOT a product the compiler could fold into the residual (cs_split16(h * scale, ...) becomes
// fma(h, scale, -hi) reading the f16 half directly): the residual written as fma(hi, m, v) with m = -1 behind an empty asm.  A multiplier
// the compiler cannot see keeps the fma (v_fma_mix_f32: 4 instructions per pair); a visible -1 turns it into two v_cvt_f32_f16 and two v_sub
__device__ __forceinline__ void cs_split16_plain(float v0, float v1, unsigned& hi, unsigned& lo) {
    float m = -1.0f;
    asm("" : "+s"(m));
    const f16x2 h = __builtin_convertvector(f32x2{v0, v1}, f16x2);
    const f16x2 l = __builtin_convertvector(f32x2{__builtin_fmaf((float)h[0], m, v0), __builtin_fmaf((float)h[1], m, v1)}, f16x2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
constexpr int CS_ROWS1 = 64;                       // rows per workgroup and row group (4 waves x 16); a wave carries RG row groups
constexpr int CS_HMAX = 128, CS_K1MAX = 28;

// ---------------------------------------------------------------------------------------------------------- row-group reductions
// the 4 coordinate lanes of a row are l, l^16, l^32, l^48.  v_permlane16_swap(vdst, src) exchanges vdst's odd 16-lane rows with src's even
// rows, v_permlane32_swap the upper half of vdst with the lower half of src (scripts/probe/swapsem.hip), so with both operands = v the
// two results are "my pair's even member" and "my pair's odd member" in every lane.  Written as inline asm: hipcc (ROCm 7.2) miscompiles
// __builtin_amdgcn_permlane{16,32}_swap(v, v) followed by op(r[0], r[1]) into op(r[0], r[0]) (scripts/probe/layout16x32.hip caught it).
// s_nop 1 = the two wait states the swap needs after a VALU write of its operands.
template <typename Op> __device__ __forceinline__ float cs_rreduce(float v, Op op) {
    float a = v, b = v;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    float c = op(a, b), e = c;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(c), "+v"(e));
    return op(c, e);
}
__device__ __forceinline__ float cs_rsum(float v) { return cs_rreduce(v, [](float a, float b) { return a + b; }); }
// the row sums of four values at once, f applied to each sum: a reduce-scatter over the two swaps (distinct operands: after
// permlane16_swap(x, y) x = {x0, y0, x2, y2} and y = {x1, y1, x3, y3} by 16-lane row, after permlane32_swap(x, y) x = {x0, x1, y0, y1} and
// y = {x2, x3, y2, y3}) leaves sum i in row i, where f runs once, then an all-gather.  6 swaps, 3 adds and 3 copies where four cs_rsum
// take 8, 8 and 8; each sum is added in cs_rsum's order (rows 0 + 1, 2 + 3, then the two), so it carries the same bits
template <typename F> __device__ __forceinline__ void cs_rsum4(float a, float b, float c, float d, F f, float (&out)[4]) {
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3" : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    float ab = a + b, cd = c + d;                                  // {a01, b01, a23, b23}, {c01, d01, c23, d23}
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(ab), "+v"(cd));
    float t = f(ab + cd), t2 = t;                                  // row i: f(sum i)
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(t), "+v"(t2));         // {A, B, A, B}, {C, D, C, D}
    float t1 = t, t3 = t2;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3" : "+v"(t), "+v"(t1), "+v"(t2), "+v"(t3));
    out[0] = t; out[1] = t1; out[2] = t2; out[3] = t3;
}
__device__ __forceinline__ float cs_rmax(float v) { return cs_rreduce(v, [](float a, float b) { return fmaxf(a, b); }); }
// the row reductions of TWO values at once (one from each row group of a wave): X = reduction of x, Y = of y, in every lane.  Distinct
// operands again, by 16-lane row: after permlane16_swap(x, y) x = {x0, y0, x2, y2} and y = {x1, y1, x3, y3}; s = op(x, y) =
// {x01, y01, x23, y23}; after permlane32_swap(s, s) s = {x01, y01, x01, y01} and s2 = {x23, y23, x23, y23}; t = op(s, s2) = {X, Y, X, Y};
// after permlane16_swap(t, t) t = {X, X, X, X} and t2 = {Y, Y, Y, Y}.  3 swaps, 2 ops and 2 copies where two cs_rreduce take 4, 4 and 4
// (x and y are consumed: hand in temporaries and the first swap needs no copy); each result is combined in cs_rreduce's order (rows
// 0 + 1, 2 + 3, then the two), so it carries the same bits
template <typename Op> __device__ __forceinline__ void cs_rreduce2(float x, float y, Op op, float& X, float& Y) {
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    float s = op(x, y), s2 = s;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(s), "+v"(s2));
    float t = op(s, s2), t2 = t;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(t), "+v"(t2));
    X = t; Y = t2;
}
__device__ __forceinline__ void cs_rsum2(float x, float y, float& X, float& Y) { cs_rreduce2(x, y, [](float a, float b) { return a + b; }, X, Y); }
__device__ __forceinline__ void cs_rmax2(float x, float y, float& X, float& Y) { cs_rreduce2(x, y, [](float a, float b) { return fmaxf(a, b); }, X, Y); }

// the lane's index in its wave, counted again by the hardware (lanes below this one): costs two instructions where it is wanted and no
// register in between, where a value kept from threadIdx.x lives through the whole kernel.  volatile: it stays where it is written
__device__ __forceinline__ int cs_lane_again() {
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}

static inline bool cs_layer_supported(const jf_gf_layer& h, int D) {
    return h.num_kde == CS_K && h.hh_iter >= 0 && h.hh_iter <= CS_HH && h.nonlinear_stretch_type == JF_GF_STRETCH_CLASSIC &&
           h.rotation_mode == JF_GF_ROT_HOUSEHOLDER && !h.center_mean && !h.add_skewness &&
           h.width_mode == JF_GF_WIDTH_SMOOTH_SATURATION && !h.clamp_widths && h.fit_normalization && h.regulate_normalization &&
           h.width_min > 0 && h.width_max > 0 && D >= 3 && D <= 4;
}

// one chunk of a packed image -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds: 1 KiB per wave instruction, no register hop): wave w of the 4 moves
// KiB pieces w, w + 4, ...; the bias tail goes with wave 0.  A plain function with the sizes as arguments (constants after inlining): the same
// builtin inside a lambda of a kernel TEMPLATE whose sizes depend on a template parameter made hipcc's host pass drop the kernel's stub
// without a diagnostic (undefined __device_stub__ symbols when the library loads).
__device__ __forceinline__ void cs_dma_chunk(__amdgpu_buffer_rsrc_t rsrc, unsigned char* dst, int g, int lane_off, int wave, int lane, int w_bytes,
                                             int b_bytes) {
#pragma unroll
    for (int u = 0; u < CS_W_BYTES / 4096; ++u)
        if (u < w_bytes / 4096) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (cs_lptr)(dst + (u * 4 + wave) * 1024), 16, lane_off, g + u * 4096, 0, 0);
    if (wave == 0 && lane < b_bytes / 16) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (cs_lptr)(dst + w_bytes), 16, lane * 16, g + w_bytes, 0, 0);
}

// ---------------------------------------------------------------------------------------------------------- phase 1
// h^T = tanh(W1 x^T + b1) for the wave's RG x 16 rows (exact f32 MFMA; rows past B replicate row B-1), returned as MFMA B operands: NP
// pieces per value (three bf16, or two f16 of h 2^14), k-slot i of lane group q in k-step s = hidden unit 16 (2 s + i / 4) + 4 q + i % 4.
// Xs: LDS scratch of (CS_ROWS1 RG + CS_HMAX) (k1p + 1) + CS_HMAX floats.  STORE_H: the f32 activations also go to h_out (B, H) -- the
// adjoint's weight-gradient product reads them.  Ends with every wave past the barrier that follows the staging, NOT past one after the
// MFMA reads: the caller's next barrier covers those.
template <int RG, bool STORE_H, int NP = CS_NP>
__device__ __forceinline__ void cs_hidden(const float* __restrict__ in, int64_t in_stride, const float* __restrict__ W1, int64_t w1s,
                                          const float* __restrict__ b1, int K1, int H, int64_t row0, int64_t last, float* Xs,
                                          bf16x8 (&hB)[RG][CS_KSTEPS][NP], float* __restrict__ h_out, int64_t hs, const CondIn* cin = nullptr) {
    using MF = Mfma16<float>;
    constexpr int CS_ROWS = CS_ROWS1 * RG;
    constexpr int MT = 16, KS = 4, JH = CS_HMAX / MT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lq = lane >> 4;
    const int k1p = (K1 + KS - 1) / KS * KS, ldk = k1p + 1;
    float* W1s = Xs + CS_ROWS * ldk;
    float* b1s = W1s + CS_HMAX * ldk;
    // f16 pairs: W1 and b1 are staged times 2 log2(e), so the matrix product below IS the v_exp_f32 argument of tanh
    constexpr float PRE = NP == 2 ? 2.8853900817779268f : 1.0f;
    // Staging, one row per thread: thread t < CS_ROWS owns input row t of the tile, the next CS_HMAX threads one hidden unit (a row of W1 and
    // its bias) each.  A thread walks its row's columns in order, eight per turn (one turn up to K1 = 8): no index division, no per-element
    // segment search, and the segment bookkeeping is scalar (CondWalk).  Every branch is wave-uniform (CS_ROWS is a multiple of 64: a wave
    // stages rows or hidden units, never both); all the global loads of a turn, and the angles of the embedded segments before the first
    // turn, are issued before the first LDS write (a load waited for inside a branch is a round trip of its own: jf_cond_in.h).
    constexpr int CG = 8;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    if (wv * 64 < CS_ROWS) {
        const int64_t avail = last - row0;
        const int64_t row = row0 + (tid <= avail ? tid : avail);   // rows past B replicate row B-1
        float ea[JF_COND_IN_MAX], eb[JF_COND_IN_MAX];
        if (cin) {
#pragma unroll
            for (int i = 0; i < JF_COND_IN_MAX; ++i) {
                if (i < cin->n && cin->s[i].kind != 0) {
                    const float* r = static_cast<const float*>(cin->s[i].src) + row * cin->s[i].stride;
                    ea[i] = r[0]; eb[i] = r[cin->s[i].kind - 1];
                }
            }
        }
        float* xr = Xs + tid * ldk;
        CondWalk w = cin ? CondWalk() : CondWalk(in, in_stride, K1, row);
        for (int c0 = 0; c0 < k1p; c0 += CG) {
            float v[CG]; bool plain[CG];
#pragma unroll
            for (int u = 0; u < CG; ++u) {
                plain[u] = false;
                if (c0 + u < K1) {
                    if (cin) w.enter(*cin, row);
                    plain[u] = w.kind == 0;
                    if (plain[u]) v[u] = *w.p;
                    w.next();
                }
            }
#pragma unroll
            for (int u = 0; u < CG; ++u) {
                if (plain[u]) xr[c0 + u] = v[u];
                else if (c0 + u >= K1 && c0 + u < k1p) xr[c0 + u] = 0.f;
            }
        }
        if (cin) {
            int off = 0;
#pragma unroll
            for (int i = 0; i < JF_COND_IN_MAX; ++i) {
                if (i < cin->n) {
                    const int kind = cin->s[i].kind;
                    if (kind != 0) {
                        // the angles become visible to the compiler only here, behind the plain columns' loads and writes: it otherwise
                        // starts the embedding's arithmetic, and waits for the angles, right behind their loads
                        asm volatile("" : "+v"(ea[i]), "+v"(eb[i]) : : "memory");
                        cond_in_embed(kind, ea[i], eb[i], xr + off);
                    }
                    off += kind == 0 ? cin->s[i].n_in : kind + 1;
                }
            }
        }
    } else if (wv * 64 < CS_ROWS + CS_HMAX) {
        const int hu = tid - CS_ROWS, hc = hu < H ? hu : H - 1;
        const float sc = hu < H ? PRE : 0.f;                        // units past H: zero weights, zero bias
        const float* wr = W1 + (int64_t)hc * w1s;
        const float b = b1[hc];
        float* ws = W1s + hu * ldk;
        for (int c0 = 0; c0 < k1p; c0 += CG) {
            float v[CG];
#pragma unroll
            for (int u = 0; u < CG; ++u)
                if (c0 + u < K1) v[u] = wr[c0 + u];
#pragma unroll
            for (int u = 0; u < CG; ++u) {
                if (c0 + u < K1) ws[c0 + u] = v[u] * sc;
                else if (c0 + u < k1p) ws[c0 + u] = 0.f;
            }
        }
        b1s[hu] = b * sc;
    }
    __syncthreads();
    // the accumulators start from the bias: register r of tile j = hidden unit 16 j + 4 lq + r.  k-steps unrolled behind uniform guards
    // (K1 <= 28: at most 7; the first always runs, so its MFMAs take the bias registers as C and no copy is made); a step's W1 fragment
    // feeds every row group
    typename MF::Acc acc[RG][JH];
#pragma unroll
    for (int j = 0; j < JH; ++j) {
        const f32x4 bias = *reinterpret_cast<const f32x4*>(b1s + j * MT + 4 * lq);
#pragma unroll
        for (int g = 0; g < RG; ++g) acc[g][j] = bias;
    }
#pragma unroll
    for (int s = 0; s < CS_K1MAX / KS; ++s) {
        if (s == 0 || s * KS < k1p) {                              // uniform
            const int kk = s * KS + lq;
            float xb[RG], wa[JH];
#pragma unroll
            for (int g = 0; g < RG; ++g) xb[g] = Xs[((wave * RG + g) * MT + li) * ldk + kk];
#pragma unroll
            for (int j = 0; j < JH; ++j) wa[j] = W1s[(j * MT + li) * ldk + kk];
#pragma unroll
            for (int j = 0; j < JH; ++j)
#pragma unroll
                for (int g = 0; g < RG; ++g) acc[g][j] = MF::mma(wa[j], xb[g], acc[g][j]);
        }
    }
#pragma unroll
    for (int g = 0; g < RG; ++g) {
        // acc[g][j][r] = pre-activation of hidden unit 16 j + 4 lq + r for row li: k-slot i of k-step s <-> (j = 2 s + i / 4, r = i % 4)
#pragma unroll
        for (int s = 0; s < CS_KSTEPS; ++s) {
            // split by truncation, two values at a time (and / sub / and / sub + one v_perm_b32 per packed pair; exact as well: 24 significant
            // bits = 3 x 8): three v_cvt_pk_bf16_f32 per value were the expensive part of this loop
            using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
            u32x4 q0, q1, q2;
#pragma unroll
            for (int i = 0; i < 8; i += 2) {
                const int j = 2 * s + (i >> 2), r = i & 3;
                if constexpr (NP == 2) {
                    // h 2^14 = 2^14 (1 - 2 / (e^{2a} + 1)) in one fma behind the reciprocal; the split takes it as it is
                    const float t0 = fmaf(-2.0f * CS_H_SCALE, __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(acc[g][j][r]) + 1.0f), CS_H_SCALE);
                    const float t1 = fmaf(-2.0f * CS_H_SCALE, __builtin_amdgcn_rcpf(__builtin_amdgcn_exp2f(acc[g][j][r + 1]) + 1.0f), CS_H_SCALE);
                    if constexpr (STORE_H) { acc[g][j][r] = t0 * (1.0f / CS_H_SCALE); acc[g][j][r + 1] = t1 * (1.0f / CS_H_SCALE); }   // exact
                    unsigned ph, pl;
                    cs_split16_plain(t0, t1, ph, pl);
                    q0[i >> 1] = ph; q1[i >> 1] = pl;
                    continue;
                }
                const float h0 = M<float>::tanh_fast(acc[g][j][r]), h1 = M<float>::tanh_fast(acc[g][j][r + 1]);
                if constexpr (STORE_H) { acc[g][j][r] = h0; acc[g][j][r + 1] = h1; }
                const unsigned a0 = __builtin_bit_cast(unsigned, h0), a1 = __builtin_bit_cast(unsigned, h1);
                const float r0 = h0 - __builtin_bit_cast(float, a0 & 0xffff0000u), r1 = h1 - __builtin_bit_cast(float, a1 & 0xffff0000u);
                const unsigned c0 = __builtin_bit_cast(unsigned, r0), c1 = __builtin_bit_cast(unsigned, r1);
                const float s0 = r0 - __builtin_bit_cast(float, c0 & 0xffff0000u), s1 = r1 - __builtin_bit_cast(float, c1 & 0xffff0000u);
                q0[i >> 1] = __builtin_amdgcn_perm(a1, a0, 0x07060302u);
                q1[i >> 1] = __builtin_amdgcn_perm(c1, c0, 0x07060302u);
                q2[i >> 1] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, s1), __builtin_bit_cast(unsigned, s0), 0x07060302u);
            }
            hB[g][s][0] = __builtin_bit_cast(bf16x8, q0); hB[g][s][1] = __builtin_bit_cast(bf16x8, q1);
            if constexpr (NP == 3) hB[g][s][2] = __builtin_bit_cast(bf16x8, q2);
        }
        if constexpr (STORE_H) {
            const int64_t r = row0 + (wave * RG + g) * MT + li;
            if (r <= last) {
#pragma unroll
                for (int j = 0; j < JH; ++j) {
                    const int c = j * MT + 4 * lq;                 // hidden units c .. c + 3 (H is a multiple of 4 on this path)
                    if (c < H) *reinterpret_cast<f32x4*>(h_out + r * hs + c) = acc[g][j];
                }
            }
        }
    }
}

}  // namespace jf
