"""The composite field's program on the host (no GPU): every validation failure of bbfmm_isosurfaces_from_fields_opts that
the host alone can reach is BBFMM_BAD_ARGUMENT with a message naming the operand or the program position, and no device
work is started; bbfmm_debug_field_program on the host against the numpy restatement bit for bit; rmt.FieldExpr compiles
to the operands and programs it should, and refuses what it cannot express.  A handle without local coefficients and a handle on a
device group need a device and are refused in tests/test_gpu_composite_field.py; handles on different devices need a
second device and have no test."""
import ctypes

import numpy as np
import pytest

import field_program_restatement as FR
import ferreus_rbf_rs_amd as F
from ferreus_rbf_rs_amd import _lib as L
from ferreus_rbf_rs_amd import rmt

EXT = np.array([0.0, 0.0, 0.0, 1.0, 1.0, 1.0])
MAX, MIN, NEG = L.FIELD_OP_MAX, L.FIELD_OP_MIN, L.FIELD_OP_NEG


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def affine_operand(c=(0.0, 1.0, 0.0, 0.0), scale=1.0, offset=0.0):
    o = L.FieldOperand()
    o.size = ctypes.sizeof(L.FieldOperand)
    o.kind, o.scale, o.offset = L.FIELD_AFFINE, scale, offset
    for a in range(4):
        o.affine[a] = c[a]
    return o


def from_fields(operands, program, n_operands=None, n_program=None, options=None):
    """(status, message) of the entry on a small lattice; the result is destroyed"""
    lib = L.load()
    arr = (L.FieldOperand * max(len(operands), 1))(*operands)
    prog = np.ascontiguousarray(program, dtype=np.int32)
    iso = np.array([0.0])
    res = ctypes.c_void_p()
    rc = lib.bbfmm_isosurfaces_from_fields_opts(arr, len(operands) if n_operands is None else n_operands, prog.ctypes.data,
                                                len(prog) if n_program is None else n_program, EXT.ctypes.data, 0.25, iso.ctypes.data, 1,
                                                None, ctypes.addressof(options) if options is not None else None, ctypes.byref(res))
    msg = lib.bbfmm_isosurface_error(res).decode() if res else ""
    if res:
        lib.bbfmm_isosurface_destroy(res)
    return rc, msg


A = affine_operand


@pytest.mark.parametrize("operands, program, names", [
    ([A(), A()], [0, MAX, 1], "position 1"),                                  # binary code on one entry
    ([A()], [NEG, 0], "position 0"),                                          # unary code on an empty stack
    ([A()] * 8, [0, 1, 2, 3, 4, 5, 6, 7, 0] + [MAX] * 8, "position 8"),       # a ninth entry
    ([A()], [0, -4], "position 1"),                                           # unknown code
    ([A(), A()], [0, 2, MAX], "position 1"),                                  # operand id out of range
    ([A(), A()], [0, 1], "position 2"),                                       # two entries left
    ([A(scale=float("nan"))], [0], "operand 0"),
    ([A(), A(offset=float("inf"))], [0, 1, MIN], "operand 1"),
    ([A(), A(c=(0.0, float("nan"), 0.0, 0.0))], [0, 1, MIN], "operand 1"),
    ([A()], [0] + [NEG] * 64, "65 codes"),                                    # more than 64 codes
])
def test_invalid_programs_and_operands_are_bad_arguments(operands, program, names):
    rc, msg = from_fields(operands, program)
    assert rc == L.BAD_ARGUMENT and names in msg, (rc, msg)


def test_too_many_operands_and_bad_handles_are_bad_arguments():
    rc, msg = from_fields([A()] * 9, [0])
    assert rc == L.BAD_ARGUMENT and "9 operands" in msg
    rng = np.random.default_rng(0)
    kp = F.KernelParams(F.FmmKernelType.LinearRbf)
    t3 = F.FmmTree(rng.random((300, 3)), 5, kp, True, True, host_only=True)
    t2 = F.FmmTree(rng.random((300, 2)), 5, kp, True, True, host_only=True)

    def tree_operand(kind, tree, axis=2):
        o = A()
        o.kind, o.axis, o.handle = kind, axis, tree._h
        return o

    rc, msg = from_fields([A(), tree_operand(L.FIELD_HEIGHT, t3)], [0, 1, MAX])      # a d = 3 handle as HEIGHT
    assert rc == L.BAD_ARGUMENT and "operand 1" in msg and "d = 2" in msg, msg
    rc, msg = from_fields([tree_operand(L.FIELD_MODEL, t2)], [0])                    # a d = 2 handle as MODEL
    assert rc == L.BAD_ARGUMENT and "operand 0" in msg and "d = 3" in msg, msg
    rc, msg = from_fields([tree_operand(L.FIELD_MODEL, t3)], [0])                    # host-only
    assert rc == L.BAD_ARGUMENT and "operand 0" in msg and "HOST_ONLY" in msg, msg
    rc, msg = from_fields([tree_operand(L.FIELD_HEIGHT, t2, axis=3)], [0])
    assert rc == L.BAD_ARGUMENT and "operand 0" in msg and "axis" in msg, msg
    rc, msg = from_fields([tree_operand(L.FIELD_AFFINE, t3)], [0])                   # an affine operand takes no handle
    assert rc == L.BAD_ARGUMENT and "operand 0" in msg
    o = A()
    o.kind = 7
    rc, msg = from_fields([o], [0])
    assert rc == L.BAD_ARGUMENT and "operand 0" in msg and "kind" in msg
    o = A()
    o.size = 8
    rc, msg = from_fields([o], [0])
    assert rc == L.BAD_ARGUMENT and "operand 0" in msg and "size" in msg


def test_options_terms_and_missing_seeds_are_refused():
    terms = L.InterpolantTerms()
    terms.size = ctypes.sizeof(L.InterpolantTerms)
    terms.d, terms.polynomial_degree, terms.k = 3, -1, 1
    opts = L.IsosurfaceOptions(ctypes.sizeof(L.IsosurfaceOptions))
    opts.terms = ctypes.addressof(terms)
    rc, msg = from_fields([A()], [0], options=opts)
    assert rc == L.BAD_ARGUMENT and "terms" in msg
    opts = L.IsosurfaceOptions(ctypes.sizeof(L.IsosurfaceOptions))
    opts.follow = 1                                                                  # follow = surface without seeds
    rc, msg = from_fields([A()], [0], options=opts)
    assert rc == L.BAD_ARGUMENT and "seeds" in msg


def debug_program(where, scale, offset, codes, V, G):
    lib = L.load()
    m, n = V.shape
    Vf = np.asfortranarray(V)
    Gf = None if G is None else np.asfortranarray(G.reshape(m, 3 * n))
    sc, of = np.ascontiguousarray(scale, dtype=np.float64), np.ascontiguousarray(offset, dtype=np.float64)
    prog = np.ascontiguousarray(codes, dtype=np.int32)
    out_v, out_g = np.full(m, np.nan), np.full((m, 3), np.nan, order="F")
    rc = lib.bbfmm_debug_field_program(where, n, sc.ctypes.data, of.ctypes.data, prog.ctypes.data, len(prog), Vf.ctypes.data,
                                       Gf.ctypes.data if Gf is not None else None, m, out_v.ctypes.data,
                                       out_g.ctypes.data if Gf is not None else None)
    return rc, out_v, (out_g if G is not None else None)


PROGRAMS = [
    ([1.0, 1.0], [0.0, 0.0], [0, 1, MAX]),
    ([1.0, 1.0], [0.0, 0.0], [0, 1, MIN]),
    ([1.0, 1.0], [-0.0, -0.0], [0, 1, MAX]),                        # (-0.0 keeps the sign of a zero operand)
    ([1.0, 1.0], [-0.0, -0.0], [0, NEG, 1, NEG, MIN, NEG]),
    ([0.3, -1.7, 2.5], [20.1, -3.3, 0.7], [0, 1, MAX, 2, NEG, MIN]),
    ([1.0, 1.0, 1.0, 1.0], [0.1, 0.2, 0.3, 0.4], [0, 1, 2, 3, MAX, MIN, MAX]),
    ([-1.0], [0.5], [0, NEG, NEG, NEG]),
]


@pytest.mark.parametrize("with_gradients", [False, True])
@pytest.mark.parametrize("case", range(len(PROGRAMS)))
def test_host_program_equals_the_restatement_bit_for_bit(case, with_gradients):
    scale, offset, codes = PROGRAMS[case]
    V, G = FR.columns(100 + case, 1000, len(scale), with_gradients)
    rc, v, g = debug_program(0, scale, offset, codes, V, G)
    assert rc == L.OK
    rv, rg = FR.program(scale, offset, codes, V, G)
    assert np.array_equal(bits(v), bits(rv))
    if with_gradients:
        assert np.array_equal(bits(g), bits(rg))
    if case == 2:                                                    # the planted zeros: the tie keeps the first operand's sign
        z = V[:, 0] == 0.0
        assert z.sum() > 100 and np.array_equal(np.signbit(v[z]), np.signbit(V[z, 0]))
        assert np.signbit(v[z]).any() and not np.signbit(v[z]).all()


def test_debug_program_refuses_an_invalid_program():
    V, _ = FR.columns(1, 10, 2, False)
    assert debug_program(0, [1.0, 1.0], [0.0, 0.0], [0, MAX], V, None)[0] == L.BAD_ARGUMENT
    assert debug_program(0, [1.0, np.nan], [0.0, 0.0], [0, 1, MAX], V, None)[0] == L.BAD_ARGUMENT
    assert debug_program(2, [1.0, 1.0], [0.0, 0.0], [0, 1, MAX], V, None)[0] == L.BAD_ARGUMENT


# ---- rmt.FieldExpr
def kinds(operands):
    return [o.kind for o in operands]


def test_field_expressions_compile_to_operands_and_programs():
    a, b, c = rmt.affine(1.0, [1, 0, 0]), rmt.affine(2.0, [0, 1, 0]), rmt.affine(3.0, [0, 0, 1])
    ops, prog = rmt.compile_expr(rmt.maximum(a, b, c))                               # folded left
    assert prog == [0, 1, MAX, 2, MAX] and kinds(ops) == [L.FIELD_AFFINE] * 3
    ops, prog = rmt.compile_expr(rmt.minimum(-rmt.maximum(a, -b), c))
    assert prog == [0, 1, NEG, MAX, NEG, 2, MIN]
    ops, prog = rmt.compile_expr((a * 2.0 - 20.0) + 1.5)
    assert prog == [0] and ops[0].scale == 2.0 and ops[0].offset == (0.0 * 2.0 - 20.0) + 1.5
    assert np.array_equal(ops[0].coefficients, [1.0, 1.0, 0.0, 0.0])
    ops, prog = rmt.compile_expr(20.0 - (a * 2.0 + 1.0))                             # a number minus an operand
    assert prog == [0] and ops[0].scale == -2.0 and ops[0].offset == 19.0
    ops, prog = rmt.compile_expr(3.0 * a)
    assert ops[0].scale == 3.0 and ops[0].offset == 0.0
    ext = [0.5, 1.0, 1.5, 2.0, 3.0, 4.0]
    ops, prog = rmt.compile_expr(rmt.box(ext))
    assert prog == [0, 1, MAX, 2, MAX, 3, MAX, 4, MAX, 5, MAX]
    assert all(np.array_equal(o.coefficients, p) for o, p in zip(ops, FR.box_planes(ext)))
    inside, outside = np.array([[1.0, 2.0, 3.0]]), np.array([[1.0, 2.0, 5.0]])
    for x, sign in ((inside, -1), (outside, 1)):
        V = np.stack([FR.affine(o.coefficients, x) for o in ops], axis=1)
        assert np.sign(FR.program([1.0] * 6, [0.0] * 6, prog, V)[0][0]) == sign      # negative inside
    ops, prog = rmt.compile_expr(rmt.maximum(a, rmt.box(ext)))
    assert len(ops) == 7 and prog[:2] == [0, 1] and prog.count(MAX) == 6
    assert rmt.compile_expr(rmt.maximum([a, b]))[1] == [0, 1, MAX]                   # a sequence is accepted


def test_refused_field_expressions_raise_value_errors():
    a, b = rmt.affine(1.0, [1, 0, 0]), rmt.affine(2.0, [0, 1, 0])
    for bad in (lambda: 1.0 - rmt.maximum(a, b), lambda: rmt.maximum(a, b) + 1.0, lambda: rmt.minimum(a, b) * 2.0, lambda: (-a) - 1.0, lambda: a + b, lambda: a * b,
                lambda: a + float("nan"), lambda: rmt.maximum(a, 1.0), lambda: rmt.maximum(), lambda: rmt.affine(0.0, [1, 2]),
                lambda: rmt.affine(float("inf"), [1, 2, 3]), lambda: rmt.box([0, 0, 0, 1, 1]), lambda: rmt.box([0, 0, 0, 1, -1, 1]),
                lambda: rmt.field("model"), lambda: rmt.height_field(None), lambda: rmt.compile_expr(a.args[0])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(ValueError):
        rmt.compile_expr(rmt.maximum(*[a] * 9))                                      # more than 8 operands
    deep = a
    for _ in range(7):
        deep = rmt.maximum(a, deep)                                                  # folded to the right: the stack grows to 8
    assert len(rmt.compile_expr(deep)[0]) == 8
    with pytest.raises(NotImplementedError):
        rmt.build_isosurface(None, [0, 0, 0, 1, 1, 1], 0.25, 0.0, a, boundary_closure=rmt.BoundaryClosure.ClosePositive)
    with pytest.raises(ValueError):
        rmt.build_isosurface(None, [0, 0, 0, 1, 1, 1], 0.25, 0.0, a)                 # follow="surface" (the default) needs seeds
    with pytest.raises(ValueError):
        rmt.build_isosurface(None, [0, 0, 0, 1, 1, 1], 0.25, 0.0, 3.0, follow="dense")
