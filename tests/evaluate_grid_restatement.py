"""numpy restatement of the grid coordinates (csrc/evaluate_grid.hpp) and of the cut of target runs into jobs of bounded
size (csrc/targets.hpp).  Every product and sum below is one rounded numpy operation, in the order the C code uses, so
the coordinates equal the host loop and the kernel bit for bit."""
import numpy as np


def grid_coords(origin, steps, shape, r0=0, n=None):
    """Rows [r0, r0 + n) of the grid in C order, (n, d): x_a = ((origin_a + i0 S[0][a]) + i1 S[1][a]) + i2 S[2][a]."""
    origin = np.asarray(origin, dtype=np.float64).reshape(-1)
    d = origin.size
    steps = np.asarray(steps, dtype=np.float64).reshape(d, d)
    shape = [int(s) for s in shape]
    total = int(np.prod(shape))
    n = total - r0 if n is None else n
    r = np.arange(r0, r0 + n, dtype=np.int64)
    idx = np.zeros((d, n), dtype=np.int64)
    for j in range(d - 1, -1, -1):
        idx[j] = r % shape[j] if shape[j] else 0
        r = r // shape[j] if shape[j] else r
    x = np.zeros((n, d))
    for a in range(d):
        s = np.full(n, origin[a])
        for j in range(d):
            s = s + idx[j].astype(np.float64) * steps[j, a]
        x[:, a] = s
    return x


def split_runs(tgt_begin, tgt_end, job_cell, cap):
    """A run of n targets starting at b becomes q = ceil(n / cap) jobs, job j = [b + floor(j n / q), b + floor((j + 1) n / q))
    with the run's cell; runs in order.  Returns (begin, end, cell) as int32 arrays."""
    ob, oe, oc = [], [], []
    for b, e, c in zip(tgt_begin, tgt_end, job_cell):
        b, n = int(b), int(e) - int(b)
        q = -(-n // cap)
        for j in range(q):
            ob.append(b + j * n // q)
            oe.append(b + (j + 1) * n // q)
            oc.append(int(c))
    return np.array(ob, dtype=np.int32), np.array(oe, dtype=np.int32), np.array(oc, dtype=np.int32)


def rotation_z(degrees, d=3):
    """(d, d) rotation about z (d = 3) or of the plane (d = 2): row j is the image of axis j"""
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    R = np.eye(d)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1] = c, s, -s, c
    return R
