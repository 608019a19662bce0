// Device self-checks exposed through the C ABI (tests/test_ops_gpu.py): claims of the form "this rewritten function returns the
// library's bits for EVERY input" are checked over all 2^32 float patterns on the GPU, which takes well under a second.
#include "common.h"

namespace w2v2 {

namespace {

// erf_select == erff and tanh_select == tanhf (common.h), bit for bit; NaN results compare equal whatever their payload.
__global__ __launch_bounds__(256) void select_forms_kernel(unsigned long long* mismatches /* [2]: erf, tanh */) {
    unsigned long long bad_erf = 0, bad_tanh = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = __uint_as_float((unsigned)i);
        const float a = erff(x), b = erf_select(x);
        if (__float_as_uint(a) != __float_as_uint(b) && !(a != a && b != b)) ++bad_erf;
        const float c = tanhf(x), d = tanh_select(x);
        if (__float_as_uint(c) != __float_as_uint(d) && !(c != c && d != d)) ++bad_tanh;
    }
    if (bad_erf) atomicAdd(&mismatches[0], bad_erf);
    if (bad_tanh) atomicAdd(&mismatches[1], bad_tanh);
}

// gelu_erf_epi (the fp32 GEMM epilogue's exact GELU) and gelu_erf_select == gelu_erf (the library erff), the same sweep and NaN rule
__global__ __launch_bounds__(256) void gelu_epilogue_kernel(unsigned long long* mismatches /* [2]: gelu_erf_epi, gelu_erf_select */) {
    unsigned long long bad_epi = 0, bad_sel = 0;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < (1ull << 32); i += stride) {
        const float x = __uint_as_float((unsigned)i);
        const float a = gelu_erf(x), b = gelu_erf_epi(x), c = gelu_erf_select(x);
        if (__float_as_uint(a) != __float_as_uint(b) && !(a != a && b != b)) ++bad_epi;
        if (__float_as_uint(a) != __float_as_uint(c) && !(a != a && c != c)) ++bad_sel;
    }
    if (bad_epi) atomicAdd(&mismatches[0], bad_epi);
    if (bad_sel) atomicAdd(&mismatches[1], bad_sel);
}

// y = gelu_erf(x) through the library erff: the reference the GEMM epilogue tests compare with
__global__ __launch_bounds__(256) void gelu_reference_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) y[i] = gelu_erf(x[i]);
}

}  // namespace

int launch_check_select_forms(unsigned long long* mismatches_dev, hipStream_t s) {
    W2V2_REQUIRE(mismatches_dev, "check_select_forms: null argument");
    W2V2_HIP_CHECK(hipMemsetAsync(mismatches_dev, 0, 2 * sizeof(unsigned long long), s));
    W2V2_LAUNCH(select_forms_kernel, dim3(4096), dim3(256), 0, s, mismatches_dev);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

int launch_check_gelu_epilogue(unsigned long long* mismatches_dev, hipStream_t s) {
    W2V2_REQUIRE(mismatches_dev, "check_gelu_epilogue: null argument");
    W2V2_HIP_CHECK(hipMemsetAsync(mismatches_dev, 0, 2 * sizeof(unsigned long long), s));
    W2V2_LAUNCH(gelu_epilogue_kernel, dim3(4096), dim3(256), 0, s, mismatches_dev);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

int launch_gelu_reference(const float* x, float* y, int64_t n, hipStream_t s) {
    W2V2_REQUIRE(x && y && n > 0, "gelu_reference: bad argument");
    const int64_t blocks = (n + 255) / 256;
    W2V2_LAUNCH(gelu_reference_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, x, y, n);
    W2V2_HIP_CHECK(hipGetLastError());
    return W2V2_OK;
}

}  // namespace w2v2
