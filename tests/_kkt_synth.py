"""TEST INFRASTRUCTURE: synthetic block maps for the device KKT module
(csrc/kkt.hip) over the (n, m, nnz) of an existing context, so that the
kernels run at block shapes the bundled models do not have -- every
k_kkt_potri<T>, the substitution path's LDS thresholds, blocks above 160
rows, one or two blocks, 2^k and 2^k + 1 blocks -- on well-conditioned
values (cond(S) < 1e2), where an error of one element is far above rounding.

mh_kkt_create checks only that the map matches the context's (n, m, nnz),
that every index is in range and that every nonzero is placed exactly once;
mh_kkt_bind_values + mh_kkt_assemble take the values from the caller.  So
the layout is a chain: the m rows split evenly over nb blocks of at most r
rows, global columns 0..nd-1 dense, block b's c local columns the global
columns nd + b (c - P) + [0, c) -- consecutive blocks share P columns -- and
the nnz nonzeros scattered over the (row, column) slots in a random order
(the gathers then really follow a_src / d_src).

LAYOUTS lists every layout the CPU and GPU tests run; reference() solves one
of them densely (refined in long double) and by both numpy restatements."""
import functools
from dataclasses import dataclass

import numpy as np

import _kkt_ref as K
from mocohip import configs
from mocohip.kkt import BlockMap

EPS = float(np.finfo(float).eps)


def synth_block_map(n, m, nnz, nb, r, c, P, nd, rng, empty_rows=1, empty_cols=1) -> BlockMap:
    """The chain layout described above.  ``empty_rows`` global rows and
    ``empty_cols`` of the chain's columns, chosen at random, get no nonzero
    at all; the columns past the chain, nd + nb (c - P) + P .. n, have none
    either."""
    n, m, nnz = int(n), int(m), int(nnz)
    if not (nb >= 1 and r >= 1 and c >= 1 and 0 <= P and nd >= 0):
        raise ValueError("bad shape")
    if 2 * P > c:
        raise ValueError("2 P > c: a global column would sit in three blocks (S not block tridiagonal)")
    step = c - P
    if nd + nb * step + P > n:
        raise ValueError(f"the chain needs {nd + nb * step + P} columns, the context has {n}")
    sizes = np.full(nb, m // nb, np.int64)
    sizes[:m % nb] += 1
    if sizes.max() > r:
        raise ValueError(f"{m} rows over {nb} blocks need r >= {sizes.max()}")
    first = np.concatenate([[0], np.cumsum(sizes)])
    rowmap = -np.ones((nb, r), np.int32)
    colmap = -np.ones((nb, c), np.int32)
    for b in range(nb):
        rowmap[b, :sizes[b]] = np.arange(first[b], first[b + 1])
        colmap[b] = nd + b * step + np.arange(c)
    dcols = np.arange(nd, dtype=np.int32)
    # rows and columns kept free of nonzeros
    free_rows = rng.choice(m, size=min(empty_rows, m), replace=False)
    free_cols = nd + rng.choice(nb * step + P, size=min(empty_cols, nb * step + P), replace=False)
    # the slots: (block, local row, local column) of real rows, then (row, dense column)
    ok = (rowmap >= 0) & ~np.isin(rowmap, free_rows)
    slot = ok[:, :, None] & ~np.isin(colmap, free_cols)[:, None, :]
    a_slots = np.flatnonzero(slot)
    dok = np.ones((m, nd), bool)
    dok[free_rows] = False
    d_slots = np.flatnonzero(dok)
    cap = len(a_slots) + len(d_slots)
    if cap < nnz:
        raise ValueError(f"{cap} slots for {nnz} nonzeros: raise c or nd")
    chosen = rng.choice(cap, size=nnz, replace=False)        # random slots, in a random order:
    a_src = -np.ones(nb * r * c, np.int32)                   # nonzero k sits in slot chosen[k]
    d_src = -np.ones(m * max(nd, 1), np.int32)
    ids = np.arange(nnz, dtype=np.int32)
    in_a = chosen < len(a_slots)
    a_src[a_slots[chosen[in_a]]] = ids[in_a]
    d_src[d_slots[chosen[~in_a] - len(a_slots)]] = ids[~in_a]
    a_src = a_src.reshape(nb, r, c)
    d_src = d_src.reshape(m, max(nd, 1))[:, :nd]
    # col2 as mocohip.kkt.block_map builds it
    col2 = -np.ones((n, 2), np.int32)
    for b in range(nb):
        cols = colmap[b].astype(np.int64)
        pos = b * c + np.arange(c)
        fresh = col2[cols, 0] < 0
        col2[cols[fresh], 0] = pos[fresh]
        col2[cols[~fresh], 1] = pos[~fresh]
    col2[dcols] = -1
    lshare = np.zeros(nb, np.int32)
    rshare = np.full(nb, step, np.int32)
    return BlockMap(nb, r, c, P, m, n, nnz, a_src, rowmap, colmap, lshare, rshare, dcols, d_src, col2)


def synth_problem(bm, rng):
    """(vals, rs, w, dc): values in [-1, 1] / sqrt(most nonzeros of a block
    row), row scales in [0.5, 2], weights in [0.1, 10] (0 on the dense
    columns), diagonal shifts in [0.5, 2] -- S's diagonal is then O(1) and
    cond(S) stays below 1e2."""
    per_row = int((bm.a_src >= 0).sum(axis=2).max())
    vals = rng.uniform(-1.0, 1.0, bm.nnz) / np.sqrt(max(per_row, 1))
    rs = rng.uniform(0.5, 2.0, bm.m)
    w = rng.uniform(0.1, 10.0, bm.n)
    w[bm.dcols] = 0.0
    dc = rng.uniform(0.5, 2.0, bm.m)
    return vals, rs, w, dc


def refined_solve(S, B, iters=3):
    """S^-1 B (S symmetric positive definite) by a float64 Cholesky solve
    refined with long-double residuals: each round gains ~1 / (cond eps)."""
    from scipy.linalg import cho_factor, cho_solve
    f = cho_factor(S, lower=True)
    Sl = S.astype(np.longdouble)
    Bl = np.asarray(B).astype(np.longdouble)
    X = cho_solve(f, B).astype(np.longdouble)
    for _ in range(iters):
        X += cho_solve(f, (Bl - Sl @ X).astype(float))
    return X


def rel_err(X, Xd):
    """max |X - Xd| / max |Xd| (Xd long double)."""
    return float(np.abs(X - Xd).max() / np.abs(Xd).max())


# ------------------------------------------------------------------------
# host contexts: (study, (n, m, nnz)) -- the shapes are those the CPU oracle
# reports (tests/test_kkt.py checks them); only they matter to a layout
# ------------------------------------------------------------------------
def _sm(N):
    return (lambda: configs.sliding_mass(N)), (6 * N + 5, 5 * N, 37 * N)


def _gait(N):
    return (lambda: configs.gait10dof18musc(N)), (132 * N + 68, 104 * N, 9604 * N)


def _ginv4():
    # the robust detection rule: device and oracle detect the same pattern
    # (the default any-change rule depends on rounding-level couplings, so
    # its nnz differs between the two)
    st = configs.gait10dof18musc_inverse(4)
    st.solver.optim_sparsity_detection_rule = "robust"
    return st


def host(name):
    """'smN' = sliding_mass(N), 'gaitN' = gait10dof18musc(N), 'ginv4' =
    gait10dof18musc_inverse(4) -> (study factory, (n, m, nnz))."""
    if name == "ginv4":
        return _ginv4, (740, 558, 3420)
    if name.startswith("sm"):
        return _sm(int(name[2:]))
    if name.startswith("gait"):
        return _gait(int(name[4:]))
    raise KeyError(name)


@dataclass(frozen=True)
class Layout:
    host: str
    nb: int
    r: int
    c: int
    P: int
    nd: int

    @property
    def paths(self):
        """The factorization paths this layout runs: both below the
        inverse path's bound (INV_RMAX = 160), the module's own choice above."""
        return ("inverse", "substitution") if self.r <= 160 else ("auto",)


def _chain(r, nb, c, P, nd=1, short=1):
    """A sliding_mass host sized to nb blocks of r rows less ``short``
    intervals' worth (5 rows each): some blocks are full, the others padded."""
    N = nb * r // 5 - short
    assert -(-5 * N // nb) <= r and N >= 1
    return Layout(f"sm{N}", nb, r, c, P, nd)


LAYOUTS = {}
# the block count: one and two blocks (no coupling product, no V, one level),
# powers of two and 2^k + 1 (the last odd block of a level without a right
# neighbour), r = 20 (potri<2>, every product of the inverse path a skinny one)
for _nb in (1, 2, 3, 4, 8, 9, 16):
    LAYOUTS[f"nb{_nb}_r20"] = _chain(20, _nb, 12, 4)
LAYOUTS["nb17_r20"] = Layout("sm64", 17, 20, 12, 4, 1)
# P = 0: S block diagonal, the coupling product has K = 0 (r = 20: a skinny
# product; r = 80: the tiled GEMM, which then has no K tile to load)
LAYOUTS["nb4_r20_P0"] = _chain(20, 4, 12, 0)
LAYOUTS["nb4_r80_P0"] = _chain(80, 4, 36, 0)
# the inverse path's register tile T = ceil(r / 16) = 1 .. 10 (r = 16, 144
# and 160 exact multiples; r = 145 .. 160 the top of the path), and the
# substitution path's LDS thresholds (k_kkt_potrf: the raised attribute from
# r = 91, LDS up to 143; k_kkt_trsm: JW = 64 up to r = 114, 32 up to 127, 16
# up to 134, 8 up to 138, L in global memory from 139)
for _r, _nb, _c, _P in ((16, 5, 12, 4), (17, 3, 20, 5), (49, 3, 40, 10), (65, 3, 36, 5), (81, 2, 40, 10),
                        (113, 3, 40, 10), (129, 3, 36, 5), (145, 3, 40, 10),
                        (90, 3, 40, 10), (91, 3, 36, 5), (114, 2, 40, 10), (115, 3, 36, 5), (127, 3, 40, 10),
                        (134, 3, 36, 5), (135, 2, 40, 10), (138, 3, 36, 5), (139, 3, 40, 10)):
    LAYOUTS[f"nb{_nb}_r{_r}"] = _chain(_r, _nb, _c, _P)
LAYOUTS["nb17_r33"] = Layout("ginv4", 17, 33, 40, 8, 2)
LAYOUTS["nb7_r45"] = Layout("gait3", 7, 45, 96, 40, 2)
LAYOUTS["nb9_r93"] = Layout("gait8", 9, 93, 100, 25, 2)
LAYOUTS["nb4_r143"] = Layout("ginv4", 4, 143, 80, 16, 2)
LAYOUTS["nb4_r144"] = Layout("ginv4", 4, 144, 80, 16, 2)
LAYOUTS["nb2_r160_dense"] = Layout("gait3", 2, 160, 100, 30, 4)
LAYOUTS["nb2_r160"] = Layout("sm64", 2, 160, 36, 5, 1)
LAYOUTS["nb5_r160"] = _chain(160, 5, 40, 10)
# above 160: substitution chosen by the module, k_kkt_potrf and k_kkt_trsm in
# global memory, the solves' products on the tiled MFMA GEMM; r = 319: the
# trsm plan without L in LDS and JW = 32
LAYOUTS["nb3_r161"] = _chain(161, 3, 36, 5)
LAYOUTS["nb5_r167"] = Layout("gait8", 5, 167, 100, 40, 3)
LAYOUTS["nb3_r190"] = Layout("ginv4", 3, 190, 150, 50, 1)
LAYOUTS["nb4_r208"] = Layout("gait8", 4, 208, 100, 50, 2)
LAYOUTS["nb1_r312"] = Layout("gait3", 1, 312, 100, 0, 2)
LAYOUTS["nb2_r319"] = _chain(319, 2, 40, 10)

WIDTHS = (1, 2, 3, 4, 7, 8, 9, 16, 17, 31, 32, 33, 64)      # every skinny NT at N = NT and N < NT, two passes


def _seed(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32)


@functools.lru_cache(maxsize=None)
def problem(name):
    """(bm, vals, rs, w, dc) of a layout, from its own seed."""
    lay = LAYOUTS[name]
    n, m, nnz = host(lay.host)[1]
    rng = np.random.default_rng(_seed(name))
    bm = synth_block_map(n, m, nnz, lay.nb, lay.r, lay.c, lay.P, lay.nd, rng)
    return (bm,) + synth_problem(bm, rng)


@dataclass
class Reference:
    S: np.ndarray          # dense_schur
    cond: float
    B: np.ndarray          # [m, max(WIDTHS)] right-hand sides
    Xd: np.ndarray         # the refined dense solve (long double)
    X: dict                # path -> the numpy restatement's solve


@functools.lru_cache(maxsize=None)
def reference(name):
    bm, vals, rs, w, dc = problem(name)
    S, _ = K.dense_schur(bm, vals, rs, w, dc)
    B = np.random.default_rng(_seed(name) + 1).standard_normal((bm.m, max(WIDTHS)))
    Xd = refined_solve(S, B)
    A, _ = K.gather(bm, vals, rs)
    D, E = K.schur_blocks(bm, A, w, dc)
    Bb = K.to_blocks(bm, B)
    f = K.cr_factor(D, E)
    X = {"substitution": K.from_blocks(bm, K.cr_solve(*f, Bb)),
         "inverse": K.from_blocks(bm, K.cr_solve(*K.cr_factor(D, E, inverse=True), Bb, inverse=True))}
    X["auto"] = X["substitution"]
    for a in (S, B, Xd, *X.values()):
        a.setflags(write=False)
    return Reference(S, float(np.linalg.cond(S)), B, Xd, X)


def solve_tolerance(ref, path, k):
    """The forward-error bound of a k-column device solve on ``path``:
    32 max(e_ref, eps cond(S)), e_ref the same path's restatement's error
    against the refined dense solve on the same columns."""
    e_ref = rel_err(ref.X[path][:, :k], ref.Xd[:, :k])
    return 32.0 * max(e_ref, EPS * ref.cond), e_ref
