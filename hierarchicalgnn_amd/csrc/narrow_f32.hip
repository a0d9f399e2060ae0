// The narrow products of the EXACT fp32 route: one side of the product is at most 32 wide (a head's last Linear, the
// encoders' 3- and 6-wide first layers).  Memory-bound fp32 VALU kernels in a fixed order, no atomics:
//
//   linear:  out[m][j] = bias[j] + sum_k x[m][k] W[j][k]          x [M, K] wide,  W [n, K],  out [M, n]
//   outer :  out[m][k] = sum_j y[m][j] W[j][k] (+ add[m][k])      y [M, n],  W [n, K],  out / add [M, K] wide
//   wgrad :  out[j][k] = sum_m y[m][j] x[m][k],  colsum[j] = sum_m y[m][j]     y [M, n],  x [M, K] wide,  out [n, K]
//
// Wide-side rows are read and written 16 bytes at a time (16-byte aligned rows, strides multiples of 4 floats); the
// narrow side (y, W, bias, out of linear, out of wgrad) is read and written one float at a time: 4-byte alignment and
// any stride that covers the width, so tab[N, 3] with its 12-byte rows is read in place.
//
// Order contracts (include/hgnn_hip.h states them, tests/exact_tail_ref.py emulates them):
//   linear: a row is shared by P = linear_lanes(K) lanes, the largest power of two <= min(K / 4, 64).  Lane t takes the
//           4-float pieces t, t + P, t + 2P, ... in that order and chains fmaf(x[k], W[j][k], acc) over its k ascending
//           from acc = 0; the P lane sums are added by a halving tree (v[t] += v[t + h] for h = P/2, P/4, .., 1); the
//           bias joins last.  A function of K only.
//   outer : acc = 0; acc = fmaf(y[m][j], W[j][k], acc) for j ascending; then out = acc + add.
//   wgrad : the rows are split into slices (wgrad_shape: a pure function of (M, n, K)); inside a slice every element
//           is the chain acc = fmaf(y[m][j], x[m][k], acc) over the slice's rows in order from acc = 0 (colsum: acc +=
//           y[m][j]); the slices are added by four chains in slice order (slices 0, 1, 2, 3 mod 4, the remainder on
//           chain 0) combined as (s0 + s1) + (s2 + s3), as hgnn_wgrad_f32 does.
#include "common.h"

namespace hgnn {
namespace nrw {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int NB = 8;   // outputs of the narrow side a thread carries at a time (n > 8: further passes / grid rows)

static int linear_lanes(int K) {
    int p = 1;
    while (p * 2 <= K / 4 && p * 2 <= 64) p *= 2;
    return p;
}

// 256 / P rows per workgroup, P lanes per row (P divides 64: a row never straddles waves)
__global__ __launch_bounds__(256) void k_linear_narrow(const float* __restrict__ x, long long ldx, long long M, int K,
                                                       const float* __restrict__ W, long long ldw,
                                                       const float* __restrict__ bias, int n, float* __restrict__ out,
                                                       long long ldo, int P) {
    const int t = threadIdx.x % P;
    const long long row = (long long)blockIdx.x * (256 / P) + threadIdx.x / P;
    const bool valid = row < M;   // no early exit: the lanes of a wave exchange their sums
    const float* xr = x + (size_t)(valid ? row : M - 1) * (size_t)ldx;
    const int nch = K / 4;
    f32x4 xv[4];   // K <= 1024: at most 4 pieces per lane (P = 64), fewer than 2 P pieces below that
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int ch = t + c * P;
        xv[c] = ch < nch ? *(const f32x4*)(xr + ch * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int j0 = 0; j0 < n; j0 += NB) {
        float acc[NB];
#pragma unroll
        for (int jj = 0; jj < NB; ++jj) acc[jj] = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int ch = t + c * P;
            if (ch < nch) {
#pragma unroll
                for (int jj = 0; jj < NB; ++jj) {
                    const int j = j0 + jj < n ? j0 + jj : n - 1;   // past n: a copy of the last output, never stored
                    const float* wp = W + (size_t)j * (size_t)ldw + ch * 4;
                    float s = acc[jj];
                    s = __builtin_fmaf(xv[c].x, wp[0], s);
                    s = __builtin_fmaf(xv[c].y, wp[1], s);
                    s = __builtin_fmaf(xv[c].z, wp[2], s);
                    s = __builtin_fmaf(xv[c].w, wp[3], s);
                    acc[jj] = s;
                }
            }
        }
        for (int h = P >> 1; h >= 1; h >>= 1) {
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) acc[jj] += __shfl_xor(acc[jj], h);
        }
        if (valid && t == 0) {
#pragma unroll
            for (int jj = 0; jj < NB; ++jj) {
                const int j = j0 + jj;
                if (j < n) out[(size_t)row * (size_t)ldo + j] = bias != nullptr ? acc[jj] + bias[j] : acc[jj];
            }
        }
    }
}

// one thread per (row, 4-float piece of the wide side)
__global__ __launch_bounds__(256) void k_outer_narrow(const float* __restrict__ y, long long ldy, long long M, int n,
                                                      const float* __restrict__ W, long long ldw, int K,
                                                      const float* __restrict__ add, float* __restrict__ out,
                                                      long long ldo) {
    const int nch = K / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= M * nch) return;
    const long long m = i / nch;
    const int k = (int)(i % nch) * 4;
    const float* yr = y + (size_t)m * (size_t)ldy;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < n; ++j) {
        const float yv = yr[j];
        const float* wp = W + (size_t)j * (size_t)ldw + k;
        acc.x = __builtin_fmaf(yv, wp[0], acc.x);
        acc.y = __builtin_fmaf(yv, wp[1], acc.y);
        acc.z = __builtin_fmaf(yv, wp[2], acc.z);
        acc.w = __builtin_fmaf(yv, wp[3], acc.w);
    }
    // `add` shares out's row stride
    if (add != nullptr) acc += *(const f32x4*)(add + (size_t)m * (size_t)ldo + k);
    *(f32x4*)(out + (size_t)m * (size_t)ldo + k) = acc;
}

struct WgradShape {
    int slices;
    long long rows_per_slice;
};

// a pure function of (M, n, K): never of the device (tests/exact_tail_ref.py restates it).  ~128 Ki threads in flight,
// one per (slice, 4-float piece of K, group of 8 narrow columns), at least 64 rows per slice.
static WgradShape wgrad_shape(long long M, int n, int K) {
    WgradShape s;
    long long want = ceil_div((long long)131072, (long long)(K / 4) * ceil_div(n, NB));
    const long long max_slices = ceil_div(M, (long long)64);
    if (want > max_slices) want = max_slices;
    if (want < 1) want = 1;
    s.rows_per_slice = ceil_div(ceil_div(M, want), (long long)16) * 16;
    if (s.rows_per_slice < 16) s.rows_per_slice = 16;
    s.slices = (int)ceil_div(M > 0 ? M : 1, s.rows_per_slice);
    return s;
}

// partial [slices][n][K + 1]: column K carries the column sum of y.  blockIdx.y = group of NB narrow columns
__global__ __launch_bounds__(256) void k_wgrad_narrow(const float* __restrict__ y, long long ldy, int n,
                                                      const float* __restrict__ x, long long ldx, int K, long long M,
                                                      float* __restrict__ partial, long long rows_per_slice, int slices) {
    const int nch = K / 4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)slices * nch) return;
    const long long slice = i / nch;
    const int k = (int)(i % nch) * 4;
    const int j0 = (int)blockIdx.y * NB;
    const long long m0 = slice * rows_per_slice;
    long long m1 = m0 + rows_per_slice;
    if (m1 > M) m1 = M;
    f32x4 acc[NB];
    float cs[NB];
#pragma unroll
    for (int jj = 0; jj < NB; ++jj) {
        acc[jj] = f32x4{0.f, 0.f, 0.f, 0.f};
        cs[jj] = 0.f;
    }
#pragma unroll 2
    for (long long m = m0; m < m1; ++m) {
        const f32x4 xv = *(const f32x4*)(x + (size_t)m * (size_t)ldx + k);
        const float* yr = y + (size_t)m * (size_t)ldy;
#pragma unroll
        for (int jj = 0; jj < NB; ++jj) {
            const float yv = yr[j0 + jj < n ? j0 + jj : n - 1];   // past n: a copy of the last column, never stored
            acc[jj].x = __builtin_fmaf(yv, xv.x, acc[jj].x);
            acc[jj].y = __builtin_fmaf(yv, xv.y, acc[jj].y);
            acc[jj].z = __builtin_fmaf(yv, xv.z, acc[jj].z);
            acc[jj].w = __builtin_fmaf(yv, xv.w, acc[jj].w);
            cs[jj] += yv;
        }
    }
    float* pp = partial + (size_t)slice * (size_t)n * (size_t)(K + 1);
#pragma unroll
    for (int jj = 0; jj < NB; ++jj) {
        const int j = j0 + jj;
        if (j < n) {
            float* pr = pp + (size_t)j * (size_t)(K + 1);
            pr[k] = acc[jj].x;
            pr[k + 1] = acc[jj].y;
            pr[k + 2] = acc[jj].z;
            pr[k + 3] = acc[jj].w;
            if (k == 0) pr[K] = cs[jj];
        }
    }
}

// the partials in slice order, hgnn_wgrad_f32's four chains; slices == 0 (no rows) writes zeros
__global__ __launch_bounds__(256) void k_wgrad_narrow_reduce(const float* __restrict__ partial, int slices, int n, int K,
                                                             float* __restrict__ out, long long ldo,
                                                             float* __restrict__ colsum) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long cnt = (long long)n * (K + 1);
    if (i >= cnt) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int s = 0;
    for (; s + 3 < slices; s += 4) {
        s0 += partial[(size_t)s * (size_t)cnt + i];
        s1 += partial[(size_t)(s + 1) * (size_t)cnt + i];
        s2 += partial[(size_t)(s + 2) * (size_t)cnt + i];
        s3 += partial[(size_t)(s + 3) * (size_t)cnt + i];
    }
    for (; s < slices; ++s) s0 += partial[(size_t)s * (size_t)cnt + i];
    const float v = (s0 + s1) + (s2 + s3);
    const int j = (int)(i / (K + 1)), k = (int)(i % (K + 1));
    if (k < K) out[(size_t)j * (size_t)ldo + k] = v;
    else if (colsum != nullptr) colsum[j] = v;
}

static bool widths_ok(int n, int K) { return n >= 1 && n <= 32 && K >= 4 && K <= 1024 && K % 4 == 0; }

}  // namespace nrw
}  // namespace hgnn

using namespace hgnn;

#define HGNN_NARROW_WIDTHS(fn, n, K)                                                                                 \
    do {                                                                                                             \
        if (!nrw::widths_ok(n, K)) {                                                                                 \
            set_error("%s: unsupported widths n=%d K=%d (1 <= n <= 32, K a multiple of 4 in [4, 1024])", fn, n, K); \
            return HGNN_ERR_UNSUPPORTED;                                                                             \
        }                                                                                                            \
    } while (0)

extern "C" int hgnn_linear_narrow_f32(const float* x, int64_t ldx, int64_t M, int32_t K, const float* W, int64_t ldw,
                                      const float* bias, int32_t n, float* out, int64_t ldo, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    static const char fn[] = "hgnn_linear_narrow_f32";
    HGNN_NARROW_WIDTHS(fn, n, K);
    HGNN_REQUIRE(M >= 0 && M <= 0x7fffffffLL, "%s: bad M", fn);
    HGNN_REQUIRE(ldx >= K && ldx % 4 == 0, "%s: ldx must be a multiple of 4 floats that covers K", fn);
    HGNN_REQUIRE(ldw >= K && ldo >= n, "%s: ldw / ldo do not cover the columns", fn);
    HGNN_REQUIRE(W != nullptr && (M == 0 || (x != nullptr && out != nullptr)), "%s: NULL pointer", fn);
    HGNN_REQUIRE((uintptr_t)x % 16 == 0, "%s: x must be 16-byte aligned", fn);
    HGNN_REQUIRE((uintptr_t)W % 4 == 0 && (uintptr_t)bias % 4 == 0 && (uintptr_t)out % 4 == 0,
                 "%s: W, bias and out must be 4-byte aligned", fn);
    if (M == 0) return HGNN_OK;
    const int P = nrw::linear_lanes(K);
    nrw::k_linear_narrow<<<(unsigned)ceil_div(M, 256 / P), 256, 0, stream>>>(x, ldx, M, K, W, ldw, bias, n, out, ldo, P);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_outer_narrow_f32(const float* y, int64_t ldy, int64_t M, int32_t n, const float* W, int64_t ldw,
                                     int32_t K, const float* add, float* out, int64_t ldo, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    static const char fn[] = "hgnn_outer_narrow_f32";
    HGNN_NARROW_WIDTHS(fn, n, K);
    HGNN_REQUIRE(M >= 0 && M <= 0x7fffffffLL, "%s: bad M", fn);
    HGNN_REQUIRE(ldo >= K && ldo % 4 == 0, "%s: ldo must be a multiple of 4 floats that covers K", fn);
    HGNN_REQUIRE(ldy >= n && ldw >= K, "%s: ldy / ldw do not cover the columns", fn);
    HGNN_REQUIRE(W != nullptr && (M == 0 || (y != nullptr && out != nullptr)), "%s: NULL pointer", fn);
    HGNN_REQUIRE((uintptr_t)out % 16 == 0 && (uintptr_t)add % 16 == 0, "%s: out and add must be 16-byte aligned", fn);
    HGNN_REQUIRE((uintptr_t)y % 4 == 0 && (uintptr_t)W % 4 == 0, "%s: y and W must be 4-byte aligned", fn);
    if (M == 0) return HGNN_OK;
    nrw::k_outer_narrow<<<(unsigned)ceil_div(M * (K / 4), 256), 256, 0, stream>>>(y, ldy, M, n, W, ldw, K, add, out, ldo);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}

extern "C" int hgnn_wgrad_narrow_f32_workspace_bytes(int64_t M, int32_t n, int32_t K, size_t* bytes) {
    static const char fn[] = "hgnn_wgrad_narrow_f32_workspace_bytes";
    HGNN_NARROW_WIDTHS(fn, n, K);
    HGNN_REQUIRE(bytes != nullptr && M >= 0 && M <= 0x7fffffffLL, "%s: bad argument", fn);
    const nrw::WgradShape s = nrw::wgrad_shape(M, n, K);
    *bytes = (size_t)s.slices * (size_t)n * (size_t)(K + 1) * sizeof(float);
    return HGNN_OK;
}

extern "C" int hgnn_wgrad_narrow_f32(const float* y, int64_t ldy, int32_t n, const float* x, int64_t ldx, int32_t K,
                                     int64_t M, float* out, int64_t ldo, float* colsum, void* workspace,
                                     size_t workspace_bytes, hgnn_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    static const char fn[] = "hgnn_wgrad_narrow_f32";
    HGNN_NARROW_WIDTHS(fn, n, K);
    HGNN_REQUIRE(M >= 0 && M <= 0x7fffffffLL, "%s: bad M", fn);
    HGNN_REQUIRE(ldx >= K && ldx % 4 == 0, "%s: ldx must be a multiple of 4 floats that covers K", fn);
    HGNN_REQUIRE(ldy >= n && ldo >= K, "%s: ldy / ldo do not cover the columns", fn);
    HGNN_REQUIRE(out != nullptr && (M == 0 || (y != nullptr && x != nullptr)), "%s: NULL pointer", fn);
    HGNN_REQUIRE((uintptr_t)x % 16 == 0, "%s: x must be 16-byte aligned", fn);
    HGNN_REQUIRE((uintptr_t)y % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)colsum % 4 == 0,
                 "%s: y, out and colsum must be 4-byte aligned", fn);
    const nrw::WgradShape s = nrw::wgrad_shape(M, n, K);
    const size_t need = (size_t)s.slices * (size_t)n * (size_t)(K + 1) * sizeof(float);
    HGNN_REQUIRE(workspace != nullptr && workspace_bytes >= need && (uintptr_t)workspace % 4 == 0,
                 "%s: workspace too small (%zu < %zu) or unaligned", fn, workspace_bytes, need);
    float* partial = (float*)workspace;
    if (M > 0) {
        const dim3 grid((unsigned)ceil_div((int64_t)s.slices * (K / 4), 256), (unsigned)ceil_div(n, nrw::NB));
        nrw::k_wgrad_narrow<<<grid, 256, 0, stream>>>(y, ldy, n, x, ldx, K, M, partial, s.rows_per_slice, s.slices);
    }
    // no rows: the reduce pass alone writes the zeros of an empty sum
    nrw::k_wgrad_narrow_reduce<<<(unsigned)ceil_div((int64_t)n * (K + 1), 256), 256, 0, stream>>>(
        partial, M > 0 ? s.slices : 0, n, K, out, ldo, colsum);
    HGNN_CHECK_HIP(hipGetLastError());
    return HGNN_OK;
}
