// Kernels of field_program.hpp: the postfix program on operand columns, the affine operand and the height operand's
// wrap, one thread per node, grid-stride over SoA columns (bandwidth-bound streaming).  No atomics, no LDS.
#include "field_program.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace bbfmm {

bool field_program_make(int32_t n_operands, const double *scale, const double *offset, const int32_t *program, int32_t n_program,
                        FieldProgram *out, std::string *err) {
    if (n_operands < 1 || n_operands > kFieldMaxOperands) {
        *err = "field program: " + std::to_string(n_operands) + " operands (1 .. " + std::to_string(kFieldMaxOperands) + ")";
        return false;
    }
    if (n_program < 1 || n_program > kFieldMaxProgram || !program) {
        *err = "field program: " + std::to_string(n_program) + " codes (1 .. " + std::to_string(kFieldMaxProgram) + ")";
        return false;
    }
    FieldProgram p;
    p.n_operands = n_operands;
    p.n_program = n_program;
    for (int o = 0; o < n_operands; ++o) {
        p.scale[o] = scale ? scale[o] : 1.0;
        p.offset[o] = offset ? offset[o] : 0.0;
        if (!std::isfinite(p.scale[o]) || !std::isfinite(p.offset[o])) {
            *err = "field program: operand " + std::to_string(o) + " has a scale or offset that is not finite";
            return false;
        }
    }
    int depth = 0;
    for (int q = 0; q < n_program; ++q) {
        const int32_t code = program[q];
        const std::string at = "field program: position " + std::to_string(q) + ": ";
        if (code >= 0) {
            if (code >= n_operands) {
                *err = at + "operand " + std::to_string(code) + " of " + std::to_string(n_operands);
                return false;
            }
            if (++depth > kFieldMaxStack) {
                *err = at + "the stack is deeper than " + std::to_string(kFieldMaxStack);
                return false;
            }
        } else if (code == kFieldOpMax || code == kFieldOpMin) {
            if (depth < 2) {
                *err = at + "stack underflow (a binary code on " + std::to_string(depth) + " entries)";
                return false;
            }
            --depth;
        } else if (code == kFieldOpNeg) {
            if (depth < 1) {
                *err = at + "stack underflow (a unary code on an empty stack)";
                return false;
            }
        } else {
            *err = at + "unknown code " + std::to_string(code);
            return false;
        }
        p.code[q] = code;
    }
    if (depth != 1) {
        *err = "field program: position " + std::to_string(n_program) + ": the program leaves " + std::to_string(depth) +
               " entries on the stack, not 1";
        return false;
    }
    *out = p;
    return true;
}

namespace {

constexpr int kThreads = 256;

int grid_for(int64_t n) {
    return static_cast<int>(std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 4096)));
}

#define FIELD_HIP(call)                                                                                                                  \
    do {                                                                                                                                 \
        if ((call) != hipSuccess) return 1;                                                                                              \
    } while (0)

__global__ __launch_bounds__(kThreads) void field_program_kernel(FieldProgram p, FieldColumns c, int64_t m, double *__restrict__ out_v,
                                                                 double *__restrict__ out_g) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
        double v, g[3];
        field_program_node(p, c, i, &v, out_g ? g : nullptr);
        out_v[i] = v;
        if (out_g)
            for (int a = 0; a < 3; ++a) out_g[a * m + i] = g[a];
    }
}

struct AffineCoefficients {
    double c[4];
};

__global__ __launch_bounds__(kThreads) void field_affine_kernel(AffineCoefficients k, const double *__restrict__ x0,
                                                                const double *__restrict__ x1, const double *__restrict__ x2, int64_t m,
                                                                double *__restrict__ vals, double *__restrict__ grad) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
        vals[i] = field_affine_value(k.c, x0[i], x1[i], x2[i]);
        if (grad)
            for (int a = 0; a < 3; ++a) grad[a * m + i] = k.c[1 + a];
    }
}

// (each thread reads and writes row i of every column only: in place)
__global__ __launch_bounds__(kThreads) void field_height_kernel(int axis, const double *__restrict__ x_axis, int64_t m, double *vals,
                                                                double *grad) {
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < m; i += (int64_t)gridDim.x * kThreads) {
        double gg[2] = {0.0, 0.0}, v, g[3];
        if (grad) {
            gg[0] = grad[i];
            gg[1] = grad[m + i];
        }
        field_height_value(axis, x_axis[i], vals[i], gg, &v, grad ? g : nullptr);
        vals[i] = v;
        if (grad)
            for (int a = 0; a < 3; ++a) grad[a * m + i] = g[a];
    }
}

} // namespace

int field_program_device(const FieldProgram &p, const FieldColumns &c, int64_t m, double *out_v, double *out_g, hipStream_t stream) {
    if (m <= 0) return 0;
    if (!out_v) return 1;
    hipLaunchKernelGGL(field_program_kernel, dim3(grid_for(m)), dim3(kThreads), 0, stream, p, c, m, out_v, out_g);
    FIELD_HIP(hipGetLastError());
    return 0;
}

int field_affine_device(const double *c, const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad,
                        hipStream_t stream) {
    if (m <= 0) return 0;
    if (!vals || !x0 || !x1 || !x2) return 1;
    AffineCoefficients k;
    for (int a = 0; a < 4; ++a) k.c[a] = c[a];
    hipLaunchKernelGGL(field_affine_kernel, dim3(grid_for(m)), dim3(kThreads), 0, stream, k, x0, x1, x2, m, vals, grad);
    FIELD_HIP(hipGetLastError());
    return 0;
}

int field_height_device(int axis, const double *x_axis, int64_t m, double *vals, double *grad, hipStream_t stream) {
    if (m <= 0) return 0;
    if (!vals || !x_axis || axis < 0 || axis > 2) return 1;
    hipLaunchKernelGGL(field_height_kernel, dim3(grid_for(m)), dim3(kThreads), 0, stream, axis, x_axis, m, vals, grad);
    FIELD_HIP(hipGetLastError());
    return 0;
}

int field_program_debug_device(const FieldProgram &p, const double *V, const double *G, int64_t m, double *out_v, double *out_g) {
    if (m <= 0) return 0;
    const size_t sm = static_cast<size_t>(m), no = static_cast<size_t>(p.n_operands);
    double *dv = nullptr, *dg = nullptr, *ov = nullptr, *og = nullptr;
    struct Free {
        double **p[4];
        ~Free() {
            for (double **q : p) (void)hipFree(*q);
        }
    } guard{{&dv, &dg, &ov, &og}};
    FIELD_HIP(hipMalloc(reinterpret_cast<void **>(&dv), sm * no * sizeof(double)));
    FIELD_HIP(hipMalloc(reinterpret_cast<void **>(&ov), sm * sizeof(double)));
    FIELD_HIP(hipMemcpy(dv, V, sm * no * sizeof(double), hipMemcpyHostToDevice));
    if (G) {
        FIELD_HIP(hipMalloc(reinterpret_cast<void **>(&dg), sm * no * 3 * sizeof(double)));
        FIELD_HIP(hipMalloc(reinterpret_cast<void **>(&og), sm * 3 * sizeof(double)));
        FIELD_HIP(hipMemcpy(dg, G, sm * no * 3 * sizeof(double), hipMemcpyHostToDevice));
    }
    FieldColumns c;
    for (size_t o = 0; o < no; ++o) {
        c.v[o] = dv + o * sm;
        c.g[o] = G ? dg + 3 * o * sm : nullptr;
        c.ldg[o] = m;
    }
    if (field_program_device(p, c, m, ov, og, nullptr) != 0) return 1;
    FIELD_HIP(hipDeviceSynchronize());
    FIELD_HIP(hipMemcpy(out_v, ov, sm * sizeof(double), hipMemcpyDeviceToHost));
    if (G) FIELD_HIP(hipMemcpy(out_g, og, sm * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

} // namespace bbfmm
