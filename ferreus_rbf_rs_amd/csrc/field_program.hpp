// A composite field over the lattice of the isosurfacer (DESIGN.md "Composite fields"): up to 8 operand columns and one
// postfix program of at most 64 codes on a stack at most 8 deep.  A code >= 0 pushes scale * v + offset of that operand
// (one multiply, then one add) with scale * grad v; MAX and MIN pop b, then a, and push the one chosen by a >= b / a <= b
// with its gradient (never fmax / fmin: the tie and the sign of zero are a's, a NaN gives b); NEG negates both.  One
// definition of the arithmetic for the host entry and the kernels of field_program.hip, never contracted to fused
// multiply-adds, as interpolant_terms.hpp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include <hip/hip_runtime_api.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define BBFMM_FIELD_HD __host__ __device__
#else
#define BBFMM_FIELD_HD
#endif

namespace bbfmm {

constexpr int kFieldMaxOperands = 8, kFieldMaxProgram = 64, kFieldMaxStack = 8;
constexpr int32_t kFieldOpMax = -1, kFieldOpMin = -2, kFieldOpNeg = -3; // BBFMM_FIELD_OP_*

struct FieldProgram {
    int n_operands = 0, n_program = 0;
    int32_t code[kFieldMaxProgram] = {};
    double scale[kFieldMaxOperands] = {}, offset[kFieldMaxOperands] = {};
};

// Operand o: its values at v[o][i]; its gradient, where asked, at g[o][a * ldg[o] + i], a = 0 .. 2.
struct FieldColumns {
    const double *v[kFieldMaxOperands] = {};
    const double *g[kFieldMaxOperands] = {};
    int64_t ldg[kFieldMaxOperands] = {};
};

// Checked copy of a caller's program (stack underflow, depth, unknown codes, operand ids, one entry left, finite scale
// and offset); false with *err naming the position or the operand.  scale / offset null: 1 / 0.
bool field_program_make(int32_t n_operands, const double *scale, const double *offset, const int32_t *program, int32_t n_program,
                        FieldProgram *out, std::string *err);

// Node i: the value, and with out_g the 3 entries of the gradient.
BBFMM_FIELD_HD inline void field_program_node(const FieldProgram &p, const FieldColumns &c, int64_t i, double *out_v, double *out_g) {
#pragma clang fp contract(off)
    double sv[kFieldMaxStack], sg[kFieldMaxStack][3];
    int top = 0;
    for (int q = 0; q < p.n_program; ++q) {
        const int32_t code = p.code[q];
        if (code >= 0) {
            const double s = p.scale[code] * c.v[code][i];
            sv[top] = s + p.offset[code];
            if (out_g)
                for (int a = 0; a < 3; ++a) sg[top][a] = p.scale[code] * c.g[code][a * c.ldg[code] + i];
            ++top;
        } else if (code == kFieldOpNeg) {
            sv[top - 1] = -sv[top - 1];
            if (out_g)
                for (int a = 0; a < 3; ++a) sg[top - 1][a] = -sg[top - 1][a];
        } else {
            const int ia = top - 2, ib = top - 1;
            const bool first = code == kFieldOpMax ? sv[ia] >= sv[ib] : sv[ia] <= sv[ib];
            if (!first) {
                sv[ia] = sv[ib];
                if (out_g)
                    for (int a = 0; a < 3; ++a) sg[ia][a] = sg[ib][a];
            }
            --top;
        }
    }
    *out_v = sv[0];
    if (out_g)
        for (int a = 0; a < 3; ++a) out_g[a] = sg[0][a];
}

// c0 + c1 x0 + c2 x1 + c3 x2, summed left to right; its gradient is (c1, c2, c3).
BBFMM_FIELD_HD inline double field_affine_value(const double *c, double x0, double x1, double x2) {
#pragma clang fp contract(off)
    double s = c[0] + c[1] * x0;
    s = s + c[2] * x1;
    s = s + c[3] * x2;
    return s;
}

// x[axis] - g, and the gradient e_axis minus grad g (gu, gv) placed on the other two axes in ascending order.
BBFMM_FIELD_HD inline void field_height_value(int axis, double x_axis, double g, const double *gg, double *out_v, double *out_g) {
#pragma clang fp contract(off)
    *out_v = x_axis - g;
    if (!out_g) return;
    const int u = axis == 0 ? 1 : 0, v = axis == 2 ? 1 : 2;
    out_g[axis] = 1.0;
    out_g[u] = -gg[0];
    out_g[v] = -gg[1];
}

// field_program.hip.  Everything here is queued on `stream` and nothing is synchronised; 0 on success.
// out_v[i] (and out_g[a * m + i]) of the program on device columns.
int field_program_device(const FieldProgram &p, const FieldColumns &c, int64_t m, double *out_v, double *out_g, hipStream_t stream);
// vals[i] = affine(x_i), grad[a * m + i] = c[1 + a] (grad may be null).
int field_affine_device(const double *c, const double *x0, const double *x1, const double *x2, int64_t m, double *vals, double *grad,
                        hipStream_t stream);
// In place: vals holds g and grad (null, or 3 columns of m whose first two hold grad g) on entry, the height field on exit.
int field_height_device(int axis, const double *x_axis, int64_t m, double *vals, double *grad, hipStream_t stream);
// The program on host columns through the device (bbfmm_debug_field_program, where = 1): V is m x n_operands, G null or
// m x 3 n_operands (operand o, axis a at column 3 o + a), both packed column-major; out_g m x 3.
int field_program_debug_device(const FieldProgram &p, const double *V, const double *G, int64_t m, double *out_v, double *out_g);

} // namespace bbfmm
