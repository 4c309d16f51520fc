"""numpy restatement of the composite field's postfix program (csrc/field_program.hpp): the pushed value is
scale * v + offset with the product rounded before the sum, MAX / MIN are np.where on >= / <= (not np.maximum: a tie keeps
the first operand with its sign of zero, a NaN gives the second), the gradient travels with the chosen value, NEG negates
both; and the affine operand's sum in its order."""
import numpy as np

OP_MAX, OP_MIN, OP_NEG = -1, -2, -3


def program(scale, offset, codes, V, G=None):
    """V: (m, n_operands); G: None or (m, n_operands, 3).  Returns values (m,) and gradients (m, 3) or None."""
    V = np.asarray(V, dtype=np.float64)
    stack = []
    for code in codes:
        if code >= 0:
            s = np.float64(scale[code]) * V[:, code]
            v = s + np.float64(offset[code])
            g = None if G is None else np.float64(scale[code]) * np.asarray(G, dtype=np.float64)[:, code, :]
            stack.append((v, g))
        elif code == OP_NEG:
            v, g = stack.pop()
            stack.append((-v, None if g is None else -g))
        else:
            (bv, bg), (av, ag) = stack.pop(), stack.pop()
            first = av >= bv if code == OP_MAX else av <= bv
            stack.append((np.where(first, av, bv), None if ag is None else np.where(first[:, None], ag, bg)))
    assert len(stack) == 1
    return stack[0]


def affine(c, x):
    """c0 + c1 x0 + c2 x1 + c3 x2, summed left to right, every product rounded first"""
    x = np.asarray(x, dtype=np.float64)
    s = np.float64(c[0]) + np.float64(c[1]) * x[:, 0]
    s = s + np.float64(c[2]) * x[:, 1]
    s = s + np.float64(c[3]) * x[:, 2]
    return s


def box_planes(extents):
    """the six affines of rmt.box in its order"""
    e = np.asarray(extents, dtype=np.float64)
    out = []
    for a in range(3):
        u = np.zeros(3)
        u[a] = 1.0
        out.append(np.concatenate([[e[a]], -u]))
        out.append(np.concatenate([[-e[3 + a]], u]))
    return out


def columns(seed, m, n_operands, gradients=True):
    """random operand columns with ties, +0 / -0 pairs and opposite values planted"""
    rng = np.random.default_rng(seed)
    V = rng.normal(size=(m, n_operands))
    G = rng.normal(size=(m, n_operands, 3)) if gradients else None
    if m >= 4 and n_operands >= 2:
        V[0::7, 1] = V[0::7, 0]              # ties
        V[1::11, 0], V[1::11, 1] = 0.0, -0.0  # a zero of either sign on both sides
        V[2::13, 0], V[2::13, 1] = -0.0, 0.0
        V[3::17, 1] = -V[3::17, 0]
    return V, G
