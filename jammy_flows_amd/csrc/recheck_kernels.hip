// The row check of checked sampling (include/jammy_hip_recheck.h): per row the largest |new - old| over the sample, the base and the log-pdf
// of a round trip, the rows beyond the tolerance as an ordered index list -- what the reference does with three masks, a column loop and a
// masked gather (extra_functions.py:464-482).  gfx950, wave64.
//
// Three launches, none of which waits for another workgroup and none of which lets an atomic decide a position:
//   flag     one thread per row: dev, the flag; the wave's flags as one 64-bit __ballot word (lane 0 stores it), the workgroup's count of
//            flagged rows (the popcounts of its four words, summed through LDS) as one 64-bit word per chunk of CHUNK rows
//   scan     ONE workgroup of SCAN_TILE threads turns the chunk counts into exclusive offsets in place, SCAN_TILE at a time with a carry,
//            and writes the total: 4096 counts at 2^20 rows (four steps).  At the row limit it walks 2^23 counts in 8192 steps, some
//            milliseconds -- beside a sampling pass of 2^31 rows that is nothing, and a second scan level would buy a fourth launch
//   scatter  one thread per row again: a flagged row's position is its chunk's offset + the popcounts of the earlier waves of its
//            workgroup + the popcount of its own wave's word below its lane.  Nothing but the words of `flag` is read
// The check is memory bound: (2 Dx + 2 Dz + 2) values per row are read once, B / 8 bytes of flag words written and read.  A lane walks its
// own row, so a wave's load covers 64 rows of one column; the rows of a wave are neighbours and every cache line that one column's load
// touches is used up by the loads of the next columns.
#include "jf_common.h"

#include "../../include/jammy_hip_recheck.h"

namespace jf {
namespace recheck {

constexpr int CHUNK = JF_RECHECK_CHUNK, WAVES = CHUNK / JF_WAVE, SCAN_TILE = JF_RECHECK_SCAN_TILE, SCAN_WAVES = SCAN_TILE / JF_WAVE;
constexpr int64_t MAX_ROWS = JF_RECHECK_MAX_ROWS;
static_assert(CHUNK % JF_WAVE == 0 && SCAN_TILE % JF_WAVE == 0, "whole waves");

// m = max(m, |b - a|) with numpy's NaN rule: once NaN, always NaN
template <typename T> __device__ __forceinline__ T max_dev(T m, T a, T b) {
    const T d = fabs(b - a);
    return (d > m || d != d) ? d : m;
}

template <typename T>
__device__ __forceinline__ T row_dev(T m, const T* __restrict__ a, const T* __restrict__ b, int32_t D) {
#pragma unroll 4
    for (int32_t k = 0; k < D; ++k) m = max_dev(m, a[k], b[k]);
    return m;
}

template <typename T>
__global__ void __launch_bounds__(CHUNK) flag_kernel(const T* __restrict__ x_old, int64_t x_old_stride, const T* __restrict__ x_new,
                                                     int64_t x_new_stride, int32_t Dx, const T* __restrict__ z_old, int64_t z_old_stride,
                                                     const T* __restrict__ z_new, int64_t z_new_stride, int32_t Dz,
                                                     const T* __restrict__ lp_old, const T* __restrict__ lp_new, int64_t B, double tol,
                                                     T* __restrict__ dev_out, unsigned long long* __restrict__ words, int64_t n_words,
                                                     int64_t* __restrict__ chunk_counts) {
    __shared__ int wave_count[WAVES];
    const int64_t b = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
    const int wave = threadIdx.x / JF_WAVE, lane = threadIdx.x % JF_WAVE;
    bool flag = false;
    if (b < B) {
        T m = max_dev((T)0, lp_old[b], lp_new[b]);
        m = row_dev(m, x_old + b * x_old_stride, x_new + b * x_new_stride, Dx);
        m = row_dev(m, z_old + b * z_old_stride, z_new + b * z_new_stride, Dz);
        flag = !((double)m <= tol);
        if (dev_out != nullptr) dev_out[b] = m;
    }
    const unsigned long long word = __ballot(flag);         // every lane of the wave is here: rows past B vote 0
    const int64_t w = (int64_t)blockIdx.x * WAVES + wave;
    if (lane == 0) {
        if (w < n_words) words[w] = word;
        wave_count[wave] = __popcll(word);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int n = 0;
#pragma unroll
        for (int i = 0; i < WAVES; ++i) n += wave_count[i];
        chunk_counts[blockIdx.x] = n;
    }
}

// counts[0 .. n) -> their exclusive prefix sums, in place; total[0] = the sum.  One workgroup.
__global__ void __launch_bounds__(SCAN_TILE) scan_kernel(int64_t* __restrict__ counts, int64_t n, int64_t* __restrict__ total) {
    __shared__ int64_t wave_sum[SCAN_WAVES];
    const int wave = threadIdx.x / JF_WAVE, lane = threadIdx.x % JF_WAVE;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += SCAN_TILE) {
        const int64_t i = base + threadIdx.x;
        const int64_t v = i < n ? counts[i] : 0;
        int64_t incl = v;                                   // inclusive scan inside the wave
#pragma unroll
        for (int off = 1; off < JF_WAVE; off <<= 1) {
            const int64_t up = __shfl_up(incl, off, JF_WAVE);
            if (lane >= off) incl += up;
        }
        if (lane == JF_WAVE - 1) wave_sum[wave] = incl;
        __syncthreads();
        int64_t before = 0, tile = 0;
#pragma unroll
        for (int k = 0; k < SCAN_WAVES; ++k) {
            const int64_t s = wave_sum[k];
            before += k < wave ? s : 0;
            tile += s;
        }
        if (i < n) counts[i] = carry + before + incl - v;
        carry += tile;
        __syncthreads();                                    // wave_sum is rewritten by the next step
    }
    if (threadIdx.x == 0) total[0] = carry;
}

__global__ void __launch_bounds__(CHUNK) scatter_kernel(const unsigned long long* __restrict__ words, int64_t n_words,
                                                        const int64_t* __restrict__ chunk_offsets, int64_t* __restrict__ idx_out) {
    const int wave = threadIdx.x / JF_WAVE, lane = threadIdx.x % JF_WAVE;
    const int64_t w0 = (int64_t)blockIdx.x * WAVES, w = w0 + wave;
    if (w >= n_words) return;
    const unsigned long long word = words[w];
    if (!(word >> lane & 1ull)) return;                     // rows past B voted 0 in flag_kernel
    int64_t pos = chunk_offsets[blockIdx.x] + __popcll(word & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; ++k) pos += __popcll(words[w0 + k]);
    idx_out[pos] = (int64_t)blockIdx.x * CHUNK + threadIdx.x;
}

// ------------------------------------------------------------------------------------------------------------ host
static int64_t chunks_of(int64_t B) { return (B + CHUNK - 1) / CHUNK; }
static int64_t words_of(int64_t B) { return (B + JF_WAVE - 1) / JF_WAVE; }

// scratch: [chunk counts / offsets: max(chunks, 1) int64][flag words: max(words, 1) uint64]
static int64_t scratch_bytes(int64_t B) {
    if (B < 0) return JF_ERR_BADARG;
    if (B > MAX_ROWS) return JF_ERR_UNSUPPORTED;
    const int64_t chunks = chunks_of(B), words = words_of(B);
    return 8 * ((chunks > 0 ? chunks : 1) + (words > 0 ? words : 1));
}

template <typename T>
static int rows(const T* x_old, int64_t x_old_stride, const T* x_new, int64_t x_new_stride, int32_t Dx, const T* z_old, int64_t z_old_stride,
                const T* z_new, int64_t z_new_stride, int32_t Dz, const T* lp_old, const T* lp_new, int64_t B, double tol, T* dev_out,
                int64_t* idx_out, int64_t* count_out, void* scratch, int64_t n_scratch, void* stream) {
    if (!lp_old || !lp_new || !idx_out || !count_out || !scratch || B < 0 || Dx < 0 || Dz < 0 || !(tol >= 0.0)) return JF_ERR_BADARG;
    if (Dx > 0 && (!x_old || !x_new || x_old_stride < Dx || x_new_stride < Dx)) return JF_ERR_BADARG;
    if (Dz > 0 && (!z_old || !z_new || z_old_stride < Dz || z_new_stride < Dz)) return JF_ERR_BADARG;
    if (B > MAX_ROWS) return JF_ERR_UNSUPPORTED;
    if (n_scratch < scratch_bytes(B)) return JF_ERR_BADARG;
    if (B == 0) return JF_OK;
    const int64_t chunks = chunks_of(B), words = words_of(B);
    int64_t* counts = (int64_t*)scratch;
    unsigned long long* flag_words = (unsigned long long*)scratch + chunks;
    hipStream_t st = (hipStream_t)stream;
    jf::launch(flag_kernel<T>, dim3((unsigned)chunks), dim3(CHUNK), 0, st, x_old, x_old_stride, x_new, x_new_stride, Dx, z_old, z_old_stride,
               z_new, z_new_stride, Dz, lp_old, lp_new, B, tol, dev_out, flag_words, words, counts);
    jf::launch(scan_kernel, dim3(1), dim3(SCAN_TILE), 0, st, counts, chunks, count_out);
    jf::launch(scatter_kernel, dim3((unsigned)chunks), dim3(CHUNK), 0, st, (const unsigned long long*)flag_words, words, (const int64_t*)counts,
               idx_out);
    return check_launch();
}

}  // namespace recheck
}  // namespace jf

extern "C" {
int jf_recheck_abi_version(void) { return 1; }
int64_t jf_recheck_scratch_bytes(int64_t B) { return jf::recheck::scratch_bytes(B); }
int jf_recheck_rows_f32(const float* x_old, int64_t x_old_stride, const float* x_new, int64_t x_new_stride, int32_t Dx, const float* z_old,
                        int64_t z_old_stride, const float* z_new, int64_t z_new_stride, int32_t Dz, const float* lp_old, const float* lp_new,
                        int64_t B, double tol, float* dev_out, int64_t* idx_out, int64_t* count_out, void* scratch, int64_t scratch_bytes,
                        void* s) {
    return jf::recheck::rows<float>(x_old, x_old_stride, x_new, x_new_stride, Dx, z_old, z_old_stride, z_new, z_new_stride, Dz, lp_old, lp_new, B,
                                    tol, dev_out, idx_out, count_out, scratch, scratch_bytes, s);
}
int jf_recheck_rows_f64(const double* x_old, int64_t x_old_stride, const double* x_new, int64_t x_new_stride, int32_t Dx, const double* z_old,
                        int64_t z_old_stride, const double* z_new, int64_t z_new_stride, int32_t Dz, const double* lp_old, const double* lp_new,
                        int64_t B, double tol, double* dev_out, int64_t* idx_out, int64_t* count_out, void* scratch, int64_t scratch_bytes,
                        void* s) {
    return jf::recheck::rows<double>(x_old, x_old_stride, x_new, x_new_stride, Dx, z_old, z_old_stride, z_new, z_new_stride, Dz, lp_old, lp_new,
                                     B, tol, dev_out, idx_out, count_out, scratch, scratch_bytes, s);
}
}
