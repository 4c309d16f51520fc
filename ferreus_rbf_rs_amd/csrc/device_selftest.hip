// Peak self-tests of the FP64 matrix and vector pipes (what bench.py quotes its roofs from), and the element-wise test
// hooks that run the kernel functions of kernels.hpp on the device.
#include <vector>

#include "device_common.hpp"

namespace bbfmm {

// ------------------------------------------------------------------ MFMA self test
// Four independent 4x4x4 products: A[b][i][k], B[b][k][j], D[b][i][j] (row-major per block).
__global__ void mfma_layout_kernel(const double *A, const double *B, double *D) {
    const int lane = threadIdx.x & 63;
    const int hi = lane >> 4, b = (lane >> 2) & 3, lo = lane & 3;
    const double a = A[(b * 4 + lo) * 4 + hi];  // A: lane = 16k + 4b + i
    const double bb = B[(b * 4 + hi) * 4 + lo]; // B: lane = 16k + 4b + j
    double c = 0.0;
    c = __builtin_amdgcn_mfma_f64_4x4x4f64(a, bb, c, 0, 0, 0);
    D[(b * 4 + hi) * 4 + lo] = c;               // D: lane = 16i + 4b + j
}

__global__ __launch_bounds__(256) void mfma_peak_kernel(double *sink, int iters, unsigned long long *stamps) {
    const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    double c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int q = 0; q < 8; ++q) c[q] = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, c[q], 0, 0, 0);
    }
    double sum = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) sum += c[q];
    if (sum == 12345.678) sink[0] = sum;
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (stamps && (threadIdx.x & 63) == 0) {
        const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        stamps[2 * w] = t1 - t0;     // shader cycles
        stamps[2 * w + 1] = r1 - r0; // 100 MHz ticks
    }
}

int mfma_f64_selftest(double *tflops, int *layout_errors, double *info) {
    double hA[64], hB[64], hD[256], ref[256];
    // exact small integers, asymmetric B (catches a transposed or block-swapped map)
    for (int b = 0; b < 4; ++b)
        for (int i = 0; i < 4; ++i)
            for (int k = 0; k < 4; ++k) {
                hA[(b * 4 + i) * 4 + k] = (double)(1 + b * 17 + i * 5 + k * 3);
                hB[(b * 4 + i) * 4 + k] = (double)(2 + b * 11 + i * 7 + k * k); // B[b][k=i][j=k]
            }
    for (int b = 0; b < 4; ++b)
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) {
                double s = 0;
                for (int k = 0; k < 4; ++k) s += hA[(b * 4 + i) * 4 + k] * hB[(b * 4 + k) * 4 + j];
                ref[(b * 4 + i) * 4 + j] = s;
            }
    double *dA = nullptr, *dB = nullptr, *dD = nullptr;
    if (hipMalloc(&dA, sizeof hA) != hipSuccess) return 1;
    if (hipMalloc(&dB, sizeof hB) != hipSuccess) return 1;
    if (hipMalloc(&dD, sizeof hD) != hipSuccess) return 1;
    (void)hipMemcpy(dA, hA, sizeof hA, hipMemcpyHostToDevice);
    (void)hipMemcpy(dB, hB, sizeof hB, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(mfma_layout_kernel, dim3(1), dim3(64), 0, 0, dA, dB, dD);
    if (hipMemcpy(hD, dD, sizeof hD, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    int errs = 0;
    for (int i = 0; i < 64; ++i)
        if (hD[i] != ref[i]) ++errs;
    *layout_errors = errs;
    // peak of v_mfma_f64_4x4x4 (512 flop): `blocks` x 4 waves, 8 independent accumulators per wave.  info[0..5]:
    //   [0] cycles per MFMA, one wave alone on a CU        [1] its shader clock (MHz)
    //   [2] cycles per MFMA per SIMD, 1 wave/SIMD, all CUs [3] clock under that load (MHz)
    //   [4] TFLOP/s at 1 wave/SIMD                          [5] TFLOP/s at 2 waves/SIMD
    const int iters = 4096;
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0);
    (void)hipEventCreate(&e1);
    unsigned long long *dS = nullptr;
    const int max_blocks = 2048;
    (void)hipMalloc(&dS, sizeof(unsigned long long) * 2 * 4 * max_blocks);
    std::vector<unsigned long long> hS(2 * 4 * max_blocks);
    auto run = [&](int blocks, int threads, double *cyc, double *mhz) {
        hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(threads), 0, 0, dD, 16, nullptr); // warm-up
        (void)hipEventRecord(e0, 0);
        hipLaunchKernelGGL(mfma_peak_kernel, dim3(blocks), dim3(threads), 0, 0, dD, iters, dS);
        (void)hipEventRecord(e1, 0);
        (void)hipEventSynchronize(e1);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e0, e1);
        const int waves = blocks * (threads / 64);
        (void)hipMemcpy(hS.data(), dS, sizeof(unsigned long long) * 2 * 4 * blocks, hipMemcpyDeviceToHost);
        double sc = 0, sr = 0;
        for (int b = 0; b < blocks; ++b)
            for (int w = 0; w < threads / 64; ++w) {
                sc += (double)hS[2 * (b * 4 + w)];
                sr += (double)hS[2 * (b * 4 + w) + 1];
            }
        if (cyc) *cyc = sc / waves / (8.0 * iters);
        if (mhz) *mhz = sr > 0 ? sc / sr * 100.0 : 0.0;
        return (double)waves * iters * 8.0 * 512.0 / (ms * 1e-3) / 1e12;
    };
    double i0 = 0, i1 = 0, i2 = 0, i3 = 0;
    run(1, 64, &i0, &i1);
    const double tf1 = run(256, 256, &i2, &i3);
    const double tf2 = run(512, 256, nullptr, nullptr);
    const double tf8 = run(2048, 256, nullptr, nullptr);
    *tflops = tf8 > tf2 ? (tf8 > tf1 ? tf8 : tf1) : (tf2 > tf1 ? tf2 : tf1);
    if (info) {
        info[0] = i0; info[1] = i1; info[2] = i2; info[3] = i3; info[4] = tf1; info[5] = tf2;
    }
    (void)hipFree(dS);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(dA);
    (void)hipFree(dB);
    (void)hipFree(dD);
    return 0;
}

// ------------------------------------------------------------------ FP64 vector-ALU peak (the pair kernels' roofline)
// Eight independent v_fma_f64 chains per lane: what the vector pipe sustains chip-wide, and at which clock (the
// FP64 load pulls the shader clock well under the 2.4 GHz of AMD's 78.6 TFLOP/s).
__global__ __launch_bounds__(256) void valu_peak_kernel(double *sink, int iters, unsigned long long *stamps) {
    double a = 1.0 + threadIdx.x * 1e-9;
    const double b = 1.0 - 1e-9;
    double c[8] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8};
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int q = 0; q < 8; ++q) c[q] = fma(c[q], b, a);
    }
    double sum = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q) sum += c[q];
    if (sum == 12345.678) sink[0] = sum;
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (stamps && (threadIdx.x & 63) == 0) {
        const size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        stamps[2 * w] = t1 - t0;
        stamps[2 * w + 1] = r1 - r0;
    }
}

// tflops: FMA flops per second chip-wide (2 per lane and instruction); mhz: the shader clock during the run.
int valu_f64_selftest(double *tflops, double *mhz) {
    const int iters = 8192, blocks = 4096;
    double *sink = nullptr;
    unsigned long long *dS = nullptr;
    if (hipMalloc(&sink, 64) != hipSuccess) return 1;
    if (hipMalloc(&dS, sizeof(unsigned long long) * 2 * 4 * blocks) != hipSuccess) {
        (void)hipFree(sink);
        return 1;
    }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        if (e0) (void)hipEventDestroy(e0);
        (void)hipFree(sink);
        (void)hipFree(dS);
        return 1;
    }
    hipLaunchKernelGGL(valu_peak_kernel, dim3(blocks), dim3(256), 0, 0, sink, 64, nullptr); // warm-up
    (void)hipEventRecord(e0, 0);
    hipLaunchKernelGGL(valu_peak_kernel, dim3(blocks), dim3(256), 0, 0, sink, iters, dS);
    (void)hipEventRecord(e1, 0);
    (void)hipEventSynchronize(e1);
    float ms = 0;
    (void)hipEventElapsedTime(&ms, e0, e1);
    std::vector<unsigned long long> hS(2 * 4 * blocks);
    (void)hipMemcpy(hS.data(), dS, sizeof(unsigned long long) * hS.size(), hipMemcpyDeviceToHost);
    double sc = 0, sr = 0;
    for (size_t w = 0; w < (size_t)4 * blocks; ++w) {
        sc += (double)hS[2 * w];
        sr += (double)hS[2 * w + 1];
    }
    *tflops = (double)blocks * 256 * iters * 8.0 * 2.0 / (ms * 1e-3) / 1e12;
    *mhz = sr > 0 ? sc / sr * 100.0 : 0.0;
    (void)hipFree(sink);
    (void)hipFree(dS);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    return 0;
}

// ------------------------------------------------------------------ element-wise test hooks (bbfmm_debug_kernel_values / _math)
// One thread per element through the device branch of kernels.hpp: the very functions the pair kernels inline.
template <int ID>
__global__ __launch_bounds__(256) void debug_kernel_values_kernel(KernelSpec ks, const double *__restrict__ r2, int64_t n,
                                                                  double *__restrict__ value, double *__restrict__ value_g,
                                                                  double *__restrict__ factor) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = r2[i];
    value[i] = kernel_value_r2<ID>(ks, x);
    double f;
    value_g[i] = kernel_value_grad_r2<ID>(ks, x, &f);
    factor[i] = f;
}

__global__ __launch_bounds__(256) void debug_math_kernel(int which, const double *__restrict__ x, int64_t n,
                                                         double *__restrict__ out, double *__restrict__ out2) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double a = 0.0, b = 0.0;
    switch (which) {
    case 0: a = bb_sqrt(x[i]); break;
    case 1: bb_sqrt_rsqrt(x[i], &a, &b); break;
    case 2: a = bb_rcp(x[i]); break;
    default: a = bb_log(x[i]); break;
    }
    out[i] = a;
    if (out2) out2[i] = b;
}

namespace {
// n_in host doubles up, n_out arrays of n doubles down; `launch` gets the device pointers (input first).
template <class Launch> int debug_elementwise(const double *in, int64_t n, double *const *outs, int n_out, Launch &&launch) {
    if (n == 0) return 0;
    const size_t bytes = sizeof(double) * (size_t)n;
    double *d[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    for (int q = 0; q <= n_out && rc == 0; ++q)
        if (hipMalloc(&d[q], bytes) != hipSuccess) rc = 1;
    if (rc == 0 && hipMemcpy(d[0], in, bytes, hipMemcpyHostToDevice) != hipSuccess) rc = 1;
    if (rc == 0) {
        launch(d);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = 1;
    }
    for (int q = 0; q < n_out && rc == 0; ++q)
        if (outs[q] && hipMemcpy(outs[q], d[q + 1], bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = 1;
    for (double *p : d)
        if (p) (void)hipFree(p);
    return rc;
}
} // namespace

int debug_kernel_values_device(const KernelSpec &ks, const double *r2, int64_t n, double *value, double *value_g, double *factor) {
    double *outs[3] = {value, value_g, factor};
    const unsigned blocks = (unsigned)((n + 255) / 256);
    return debug_elementwise(r2, n, outs, 3, [&](double **d) {
        dispatch_kernel_id(ks.id, [&](auto idc) {
            hipLaunchKernelGGL((debug_kernel_values_kernel<decltype(idc)::value>), dim3(blocks), dim3(256), 0, 0, ks, d[0], n, d[1],
                               d[2], d[3]);
        });
    });
}

int debug_math_device(int which, const double *x, int64_t n, double *out, double *out2) {
    double *outs[2] = {out, out2};
    const unsigned blocks = (unsigned)((n + 255) / 256);
    return debug_elementwise(x, n, outs, 2, [&](double **d) {
        hipLaunchKernelGGL(debug_math_kernel, dim3(blocks), dim3(256), 0, 0, which, d[0], n, d[1], out2 ? d[2] : nullptr);
    });
}

} // namespace bbfmm
