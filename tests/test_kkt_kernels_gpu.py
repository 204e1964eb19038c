"""The kernels of csrc/kkt.hip at their size edges, on the synthetic block
maps of tests/_kkt_synth.py (tests/test_kkt.py checks the layouts and both
numpy restatements without a GPU): every k_kkt_potri<T>, the top of the
inverse path (r = 145 .. 160), the substitution path's LDS thresholds
(k_kkt_potrf, every trsm plan), blocks above 160 rows (substitution chosen by
the module, everything in global memory, the solves' products on the tiled
GEMM), 1, 2, 2^k and 2^k + 1 blocks, every k_kkt_gemm_skinny<NT> at N = NT
and N < NT -- on systems of cond(S) < 1e2, so the bounds are those of
rounding: a wrong element of one tile is orders of magnitude above them.

The device's values come from the test (mh_kkt_bind_values of a torch tensor
+ mh_kkt_assemble), not from the host context's Jacobian: the context only
supplies (n, m, nnz), which is all mh_kkt_create ties a block map to."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import _kkt_ref as K
import _kkt_synth as SY
from mocohip.kkt import DeviceKKT
from mocohip.solver import HipNLP

pytestmark = pytest.mark.gpu

EPS = SY.EPS
PATH_CASES = [(name, path) for name in sorted(SY.LAYOUTS) for path in SY.LAYOUTS[name].paths]


@pytest.fixture(scope="module")
def hosts():
    """The host contexts, one per shape, shared by the module's tests."""
    made = {}

    def get(name):
        if name not in made:
            make, shape = SY.host(name)
            st = make()
            nlp = HipNLP(st.problem.create_rep(), st.solver.options())
            assert (nlp.n, nlp.m, nlp.nnz) == shape
            made[name] = nlp
        return made[name]

    yield get
    for nlp in made.values():
        nlp.close()


class Synth:
    """DeviceKKT over a host context with a synthetic block map and the
    test's own values, row-scaled and assembled."""

    def __init__(self, nlp, bm, vals, rs, path=None, graphs=None, monkeypatch=None):
        import torch
        self.torch = torch
        if path in ("inverse", "substitution"):
            monkeypatch.setenv("MOCOHIP_KKT_INV", "1" if path == "inverse" else "0")
        elif monkeypatch is not None:
            monkeypatch.delenv("MOCOHIP_KKT_INV", raising=False)
        if graphs is not None:
            monkeypatch.setenv("MOCOHIP_KKT_GRAPHS", "1" if graphs else "0")
        self.dk = DeviceKKT(nlp, bm)
        self.dev = torch.device("cuda", int(nlp.opts.device))
        self.dk.set_row_scale(rs)
        self.set_values(vals)

    def set_values(self, vals):
        # (the tensor stays alive until close: the module reads it on every assemble)
        self.vals = self.torch.tensor(np.ascontiguousarray(vals, float), dtype=self.torch.float64, device=self.dev)
        self.torch.cuda.synchronize(self.dev)
        dk = self.dk
        dk._check(dk.lib.mh_kkt_bind_values(dk.h, C.c_void_p(self.vals.data_ptr())))
        dk._check(dk.lib.mh_kkt_assemble(dk.h))

    def __enter__(self):
        return self.dk

    def __exit__(self, *exc):
        self.dk.close()
        self.vals = None


def _backward_error(S, X, B):
    """max |S X - B| / (|S| |X| + |B|), the residual in long double (its
    own rounding stays out of the bound; the scale needs no such care)."""
    resid = S.astype(np.longdouble) @ np.asarray(X).astype(np.longdouble) - B
    return float((np.abs(resid) / (np.abs(S) @ np.abs(X) + np.abs(B))).max())


def _check_solves(dk, name, path, widths=SY.WIDTHS):
    """Every width's solve against the refined dense solve, held to
    32 max(e_ref, eps cond(S)) forward and 64 r eps backward, each figure
    printed before it is asserted; returns {k: X} (for the determinism checks)."""
    bm = SY.problem(name)[0]
    ref = SY.reference(name)
    out, worst = {}, (0.0, 0.0)
    for k in widths:
        B = ref.B[:, 0] if k == 1 else ref.B[:, :k]
        X = dk.solve(B)
        assert X.shape == B.shape
        out[k] = X
        tol, e_ref = SY.solve_tolerance(ref, path, k)
        err = SY.rel_err(X.reshape(bm.m, -1), ref.Xd[:, :k])
        bwd = _backward_error(ref.S, X.reshape(bm.m, -1), ref.B[:, :k])
        print(f"{name} [{path}] k={k}: device error {err:.2e} (restatement {e_ref:.2e}, bound {tol:.2e}, "
              f"cond {ref.cond:.1f}), backward error {bwd:.2e} (bound {64 * bm.r * EPS:.2e})")
        worst = max(worst, (err, tol))
        assert err <= tol, (k, err, tol)
        assert bwd <= 64 * bm.r * EPS, (k, bwd)
    print(f"{name} [{path}]: largest device error {worst[0]:.2e}, bound {worst[1]:.2e}")
    return out


@pytest.mark.parametrize("name", sorted(SY.LAYOUTS))
def test_gathers_and_products(name, hosts):
    """k_kkt_gather / _gather_dense / _csr_vals, k_kkt_spmv and
    k_kkt_jtmul_dense over a map whose nonzeros sit in random slots in a
    random order, with an empty row, empty columns and columns past the
    chain: the dense columns bit for bit, the products to 1e-13 (a row sums
    at most ~250 terms of magnitude <= 2; only the order of the sum differs)."""
    bm, vals, rs, w, dc = SY.problem(name)
    with Synth(hosts(SY.LAYOUTS[name].host), bm, vals, rs) as dk:
        cols, Jd = dk.dense_columns()
        assert np.array_equal(cols, bm.dcols)
        want = np.where(bm.d_src >= 0, vals[bm.d_src] * rs[:, None], 0.0)
        assert np.array_equal(Jd, want)
        # J from the map itself: (row, column) of every nonzero
        row = np.empty(bm.nnz, np.int64)
        col = np.empty(bm.nnz, np.int64)
        b, i, j = np.nonzero(bm.a_src >= 0)
        row[bm.a_src[b, i, j]], col[bm.a_src[b, i, j]] = bm.rowmap[b, i], bm.colmap[b, j]
        i, d = np.nonzero(bm.d_src >= 0)
        row[bm.d_src[i, d]], col[bm.d_src[i, d]] = i, bm.dcols[d]
        J = sp.csr_matrix((vals * rs[row], (row, col)), shape=(bm.m, bm.n))
        assert (np.diff(J.indptr) == 0).any() and (np.diff(J.tocsc().indptr) == 0).any()
        rng = np.random.default_rng(7)
        for k in (1, 3, 32, 33):
            V = rng.uniform(-1.0, 1.0, (bm.n, k))
            Y = rng.uniform(-1.0, 1.0, (bm.m, k))
            for got, ref in ((dk.jmul(V), J @ V), (dk.jtmul(Y), J.T @ Y)):
                assert np.abs(got - ref).max() <= 1e-13 * (np.abs(ref).max() + 1.0), k
        assert np.array_equal(dk.jmul(V[:, 0]), dk.jmul(V[:, :1])[:, 0])      # a vector is one column


@pytest.mark.parametrize("name,path", PATH_CASES)
def test_factor_and_solve(name, path, hosts, monkeypatch):
    """Factor and solve against the refined dense solve of dense_schur, every
    solve width, both paths up to r = 160 and the module's own choice above;
    a second factor + solve gives the same bits."""
    bm, vals, rs, w, dc = SY.problem(name)
    with Synth(hosts(SY.LAYOUTS[name].host), bm, vals, rs, path, monkeypatch=monkeypatch) as dk:
        assert dk.factor(w, dc)
        first = _check_solves(dk, name, path)
        assert dk.factor(w, dc)
        B = SY.reference(name).B
        for k in (1, 9, 33):
            assert np.array_equal(dk.solve(B[:, 0] if k == 1 else B[:, :k]), first[k]), k


@pytest.mark.parametrize("name,path", [("nb5_r160", "inverse"), ("nb9_r93", "substitution"), ("nb5_r167", "auto")])
def test_graph_replay_matches_direct_launches(name, path, hosts, monkeypatch):
    """MOCOHIP_KKT_GRAPHS=0 (every kernel launched directly) gives the bits
    of the captured graphs' replay: the kernels are deterministic."""
    bm, vals, rs, w, dc = SY.problem(name)
    B = SY.reference(name).B
    got = []
    for graphs in (True, False):
        with Synth(hosts(SY.LAYOUTS[name].host), bm, vals, rs, path, graphs, monkeypatch) as dk:
            assert dk.factor(w, dc)
            got.append([dk.solve(B[:, :k]) for k in (1, 5, 32, 64)])
            got[-1] += [dk.solve(B[:, :5])]          # the replay of a graph captured above
    for a, b in zip(*got):
        assert np.array_equal(a, b)
    assert np.array_equal(got[0][1], got[0][-1])


FLAG_LAYOUT = "nb5_r160"


def _indefinite_block(bm, w, dc, b):
    """Negative weights on block b's own (unshared) columns and dc = 1e-8 on
    its rows: D_b is indefinite, its neighbours stay positive definite
    (-0.05: small enough that D_b's first diagonal entries stay positive)."""
    w, dc = w.copy(), dc.copy()
    w[bm.colmap[b, bm.nshare:bm.c - bm.nshare]] = -0.05
    dc[bm.rowmap[b][bm.rowmap[b] >= 0]] = 1e-8
    return w, dc


@pytest.mark.parametrize("path", ["inverse", "substitution"])
def test_failure_flag(path, hosts, monkeypatch):
    """One interior block indefinite -- block 2 of 5, eliminated at the
    second level (level 0 takes blocks 1 and 3), so the flag comes from a
    later level's launch and a later pivot than pivot 0 of level 0 -- and
    then one NaN among a block's values: factor reports False without a
    fault, solve refuses, and a refactor of the sound system meets the
    solve bound."""
    name = FLAG_LAYOUT
    bm, vals, rs, w, dc = SY.problem(name)
    assert bm.nb == 5
    wbad, dcbad = _indefinite_block(bm, w, dc, 2)
    A, _ = K.gather(bm, vals, rs)
    D, E = K.schur_blocks(bm, A, wbad, dcbad)
    assert all(np.linalg.eigvalsh(D[b]).min() > 0 for b in (1, 3))       # level 0 succeeds
    assert D[2][0, 0] > 0 and np.linalg.eigvalsh(D[2]).min() < 0         # level 1 fails past pivot 0
    with pytest.raises(np.linalg.LinAlgError):
        K.cr_factor(D, E)
    with Synth(hosts(SY.LAYOUTS[name].host), bm, vals, rs, path, monkeypatch=monkeypatch) as dk:
        assert not dk.factor(wbad, dcbad)
        with pytest.raises(RuntimeError):
            dk.solve(np.ones(bm.m))
        assert dk.factor(w, dc)                                            # recovers
        _check_solves(dk, name, path, widths=(1, 33))
    # a non-finite pivot
    vnan = vals.copy()
    k = int(bm.a_src[2][bm.a_src[2] >= 0][7])
    vnan[k] = np.nan
    syn = Synth(hosts(SY.LAYOUTS[name].host), bm, vnan, rs, path, monkeypatch=monkeypatch)
    with syn as dk:
        assert not dk.factor(w, dc)
        with pytest.raises(RuntimeError):
            dk.solve(np.ones(bm.m))
        syn.set_values(vals)
        assert dk.factor(w, dc)
        _check_solves(dk, name, path, widths=(1, 33))
