"""k_interval's overlapped order (the early Jacobian entries assembled while
the combine lanes run the solve chain) against the plain order of the same
kernel (MOCOHIP_IV_OVERLAP=0): the same bits, on the smallest shapes that
take every branch -- the first interval with the endpoint head, an interior
one, the last with its tail, a shard without head or tail, backward and
central differences (the mirror lane), path-constraint entries (CT_PATH),
kinematic-constraint outputs (late: they read udot) with the midpoint slack
words, implicit residuals with the NACC constants, two points per interval,
a model without copies (constants only) and parameter columns (CT_GEN).

The host classification behind the two entry lists is checked without a
device through mh_debug_interval_overlap."""
import ctypes as C
import os

import numpy as np
import pytest

from mocohip import abi, configs
from mocohip.solver import HipNLP, OracleNLP

CT_OFF, CT_GEN, CT_PATH = 0xFFFFF, 1 << 27, 1 << 28


def _central(st):
    st.solver.optim_finite_difference_scheme = "central"
    return st


# name -> (study, shard or None, the default context takes the overlapped order)
CASES = {
    "gait_rigid_forward_n3": (lambda: configs.gait10dof18musc(3), None, True),
    "gait_rigid_forward_n3_shard_1_2": (lambda: configs.gait10dof18musc(3), (1, 2), True),
    "gait_rigid_backward_n2": (lambda: configs.gait10dof18musc(2, fd_scheme="backward"), None, True),
    "gait_rigid_pathcon_n2": (lambda: configs.gait10dof18musc(2, control_bounds=True), None, True),
    "coupled_pendulum_n3": (lambda: configs.double_pendulum_coupled(3), None, True),
    "double_pendulum_implicit_hs_n3": (lambda: configs.double_pendulum(3, dynamics="implicit"), None, True),
    "double_pendulum_trap_n3": (lambda: configs.double_pendulum(3, "trapezoidal"), None, True),
    "double_pendulum_central_n3": (lambda: _central(configs.double_pendulum(3)), None, True),
    "sliding_mass_n2": (lambda: configs.sliding_mass(2), None, True),
    # (a model with MocoParameters runs the device interpreter, which has no
    # fused interval kernel: the flag is absent on both sides)
    "oscillator_mass_parameter_n2": (lambda: configs.oscillator_mass(2), None, False),
}


def _create(rep, opts, overlap):
    saved = os.environ.pop("MOCOHIP_IV_OVERLAP", None)
    if not overlap:
        os.environ["MOCOHIP_IV_OVERLAP"] = "0"
    try:
        return HipNLP(rep, opts)
    finally:
        os.environ.pop("MOCOHIP_IV_OVERLAP", None)
        if saved is not None:
            os.environ["MOCOHIP_IV_OVERLAP"] = saved


def _iterates(nlp, rep):
    """Two seeded iterates; a muscle model's states and controls in the
    muscles' working range (tests/test_gpu_parity.py)."""
    out = []
    for seed in (0, 1):
        r = np.random.default_rng(seed)
        x = nlp.random_iterate(r.uniform(-1, 1, nlp.n))
        if any(n.endswith("/activation") for n in rep.state_names):
            G, NS, NC = nlp.G, nlp.NS, nlp.NC
            x[2:2 + NS * G] = r.uniform(0.05, 0.5, NS * G)
            x[2 + NS * G:2 + (NS + NC) * G] = r.uniform(0.05, 0.4, NC * G)
            x[2 + (NS + NC) * G:] = r.uniform(-0.5, 0.5, nlp.n - 2 - (NS + NC) * G)
        out.append(x)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_overlapped_order_bit_identical_to_plain_order(name):
    mk, shard, takes = CASES[name]
    st = mk()
    rep = st.problem.create_rep()
    opts = st.solver.options(*shard) if shard else st.solver.options()
    on, off = _create(rep, opts, True), _create(rep, opts, False)
    fresh_on, fresh_off = _create(rep, opts, True), _create(rep, opts, False)
    try:
        assert ("interval" in on.backend_flags().split()) == takes, on.backend_flags()
        assert ("iv-overlap" in on.backend_flags().split()) == takes, on.backend_flags()
        assert "iv-overlap" not in off.backend_flags().split(), off.backend_flags()
        xs = _iterates(on, rep)
        # eval_jac_g as the first call of a fresh context
        assert np.array_equal(fresh_on.eval_jac_g(xs[0]), fresh_off.eval_jac_g(xs[0]), equal_nan=True)
        for x in xs:
            a, b = on.eval_jac_g(x), off.eval_jac_g(x)
            assert np.isfinite(b).mean() >= 0.99, np.isfinite(b).mean()
            assert np.array_equal(a, b, equal_nan=True), int((a != b).sum())
            (ga, va), (gb, vb) = on.eval_g_jac_g(x), off.eval_g_jac_g(x)
            assert np.array_equal(ga, gb, equal_nan=True), int((ga != gb).sum())
            assert np.array_equal(va, vb, equal_nan=True), int((va != vb).sum())
            assert np.array_equal(va, a, equal_nan=True)
    finally:
        for n in (on, off, fresh_on, fresh_off):
            n.close()


def _classes(st):
    rep, opts = st.problem.create_rep(), st.solver.options()
    lib = abi.load_mocohip()
    info = np.zeros(8, np.int32)
    ip = info.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.mh_debug_interval_overlap(C.byref(rep.struct), C.byref(opts), ip, None, None, None, None, 0)
    assert rc == 0, lib.mh_last_error().decode()
    nw, no = int(info[0]), int(info[3])
    cap = max(nw, no)
    words, bases = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
    early, out_early = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    u32, u8 = C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    rc = lib.mh_debug_interval_overlap(C.byref(rep.struct), C.byref(opts), ip, words.ctypes.data_as(u32),
                                       bases.ctypes.data_as(u32), early.ctypes.data_as(u8),
                                       out_early.ctypes.data_as(u8), cap)
    assert rc == 0, lib.mh_last_error().decode()
    keys = ("nw", "nnz_int", "npts", "NO", "stride", "ND", "fd", "base")
    return dict(zip(keys, map(int, info))), words[:nw], bases[:nw], early[:nw].astype(bool), out_early[:no].astype(bool)


@pytest.mark.parametrize("name", ["gait_rigid_forward_n3", "coupled_pendulum_n3"])
def test_host_classification(name):
    """Every entry is early or late and not both (one class per entry);
    an early entry and its base (mirror) word read a constant or an
    OUT_EARLY output; CT_GEN, CT_PATH and solved-output entries are late."""
    I, words, bases, early, out_early = _classes(CASES[name][0]())
    nw, stride, NO = I["nw"], I["stride"], I["NO"]
    nyall = I["npts"] * NO * stride
    late = ~early
    assert early.shape == (nw,) and (early ^ late).all() and early.sum() + late.sum() == nw
    off = (words & CT_OFF).astype(np.int64)
    special = (words & (CT_GEN | CT_PATH)) != 0

    def ready(o):
        o = np.asarray(o, np.int64)
        return (o >= nyall) | out_early[np.minimum(o // stride, I["npts"] * NO - 1) % NO]
    lane = ~special & (off < nyall)
    assert ready(off[early]).all()
    assert ready(bases[early & lane]).all()
    assert not special[early].any()
    # the base word is the base lane of the word's own (point, output) row
    assert np.array_equal(bases[lane].astype(np.int64), off[lane] // stride * stride + I["base"])
    assert (bases[~lane] == 0).all()
    solved = lane & ~out_early[(off // stride) % NO]
    assert late[special].all() and late[solved].all()
    # and nothing else is late
    assert np.array_equal(late, special | solved)
    if name.startswith("gait_rigid"):
        # an interior interval: the 18 activation rows are dense over the
        # inputs of its three points (2 x 66 + 1 + 3 x 66 columns), read
        # copies only, and are early; the 10 solved outputs are late
        assert NO == 28 and out_early.tolist() == [False] * 10 + [True] * 18
        # (the rows from the oracle's structure: an interval's rows are its
        # Hermite then its Simpson defect rows, one per state, then the
        # control-interpolation rows; the "+ 1" is the Hermite row's midpoint
        # identity, an LDS constant)
        st = CASES[name][0]()
        ref = OracleNLP(st.problem.create_rep(), st.solver.options())
        try:
            ir, _ = ref.jac_structure()
            N, nnz_int = ref.opts.num_mesh_intervals, I["nnz_int"]
            assert ref.NEP == 0 and ref.tail_rows == 0 and ref.NK == 0 and ref.NPC == 0
            rpi = ref.m // N
            # (then the NC control-interpolation rows)
            assert rpi == 2 * ref.NS + ref.NC and ref.nnz == N * nnz_int + (nw - nnz_int)
            rows = np.asarray(ir[nnz_int:2 * nnz_int]) - rpi   # interval 1 of 0..2
            assert rows.min() == 0 and rows.max() == rpi - 1
            act = (rows < 2 * ref.NS) & ((rows % ref.NS) >= 2 * ref.NQ)
        finally:
            ref.close()
        # every entry of the activation rows but their t0 / tf columns (CT_GEN)
        assert int((act & early[:nnz_int]).sum()) == 18 * (2 * 66 + 1 + 3 * 66) == 5958
        assert np.array_equal(act & late[:nnz_int], act & special[:nnz_int])
        assert int((act & special[:nnz_int]).sum()) == 2 * 18 * 2
        assert int((early[:nnz_int] & lane[:nnz_int]).sum()) == 18 * 5 * 66
        # late: the t0 / tf columns of the 2 NS defect rows, the 10 speed rows
        assert int(special[:nnz_int].sum()) == 2 * 2 * 38
        assert int(solved[:nnz_int].sum()) == 10 * (2 * 66 + 1 + 3 * 66) - 10
    else:
        # no output of the coupled pendulum copies a group result: its
        # kinematic-constraint outputs read udot; the early list is constants
        assert not out_early.any()
        assert (off[early] >= nyall).all() and early.any()
