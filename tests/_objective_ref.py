"""The objective and the gradient the objective kernels define (k_integrand,
k_grad, goal_integrand, k_reduce_obj, k_marker_final), restated in
numpy.longdouble from the Python MocoProblem and ProblemRep alone (test
helper): no call into the oracle or the library, no read of the lowered term
arrays.  Goals, term indices and weights are resolved here from
``st.problem.goals``, ``rep.state_names`` and ``rep.control_names``.

What is restated is the kernels' definition, not the analytic gradient: the
forward / backward / central quotient of the integrand at the same
double-rounded perturbed inputs fl(s +- h) and fl(t +- h seed); everything
after those inputs is long double.

Beside each value runs a bound A: the same sums with every product and term
replaced by its absolute value (the magnitudes that cancel in a tracking
difference, both legs of a quotient), and a tolerance numerator T = sum of
K_g A_g, K_g twice the count of roundings on the longest dependency path of
the device code that computes goal g's share (``roundings`` below, counted
from csrc/core.hpp goal_integrand / k_integrand / k_grad and
csrc/mocohip.hip k_reduce_obj / k_marker_final).  A test asserts
|device - reference| <= eps T."""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

import _lanes
from mocohip import abi
from mocohip.problem import (ImplicitAuxiliaryDerivativesTerm, MocoControlGoal, MocoFinalTimeGoal,
                             MocoInitialActivationGoal, MocoMarkerFinalGoal, MocoStateTrackingGoal,
                             MocoSumSquaredStateGoal)
from mocohip.solver import _NLPBase

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is not wider than double here"


class Layout(_NLPBase):
    """The sizes and the per-point gather of an NLP from its ProblemRep and
    options alone: _NLPBase's properties without a library context."""

    def __init__(self, rep, opts):
        self.rep, self.opts, self.ctx = rep, opts, None
        N = int(opts.num_mesh_intervals)
        self.G = 2 * N + 1 if opts.transcription == abi.MH_HERMITE_SIMPSON else N + 1
        self.NS, self.NC, self.NQ = rep.num_states, rep.num_controls, rep.nq
        self.n = 2 + (self.NS + self.NC + self.NDV + self.NM) * self.G + self.NSL * N + self.NPAR

    def close(self):
        pass


class Table:
    """A compiled model table: breaks and per-segment polynomial coefficients
    in t - break, lowest order first."""

    def __init__(self, rep, name):
        ms = rep.compiled.struct
        T = ms.tables[rep.compiled.table_index[name]]
        self.columns = list(rep.compiled.table_columns[name])
        self.nseg, self.ncol, self.degree = int(T.nseg), int(T.ncol), int(T.degree)
        self.br = np.array(ms.table_breaks[T.break_begin:T.break_begin + self.nseg + 1], float)
        n = self.degree + 1
        cf = np.array(ms.table_coefs[T.coef_begin:T.coef_begin + self.nseg * self.ncol * n], float)
        self.cf = cf.reshape(self.nseg, self.ncol, n).astype(LD)

    def segment(self, t):
        """The segment that holds t; the end segments extrapolate
        (table_eval, csrc/dae_device.hpp)."""
        s = np.searchsorted(self.br, t, side="right") - 1
        s = np.where(t <= self.br[0], 0, s)
        return np.where(t >= self.br[-1], self.nseg - 1, s)

    def eval(self, cols, t):
        """Columns cols at the double times t [G]: value, the sum of
        |c_k| |dt|^k, and the time derivative, each [G, len(cols)]."""
        t = np.asarray(t, float)
        s = self.segment(t)
        dt = (t.astype(LD) - self.br[s].astype(LD))[:, None]
        c = self.cf[s][:, np.asarray(cols, int), :]
        v, a, d = c[..., self.degree], np.abs(c[..., self.degree]), np.zeros_like(c[..., 0])
        for k in range(self.degree - 1, -1, -1):   # Horner
            d = d * dt + v
            v = v * dt + c[..., k]
            a = a * np.abs(dt) + np.abs(c[..., k])
        return v, a, d


@dataclass
class Goal:
    kind: str
    name: str
    W: float
    idx: np.ndarray = field(default_factory=lambda: np.zeros(0, int))    # per-point input of each term
    w: np.ndarray = field(default_factory=lambda: np.zeros(0))          # weight of each term
    exponent: int = 2
    signed: bool = False            # a mutation: v^p where the goal says |v|^p
    table: Optional[Table] = None
    cols: Optional[np.ndarray] = None
    marker: Optional[tuple] = None  # (body, location, reference location)


def resolve_goals(st, rep, nlp) -> List[Goal]:
    """The goals in the device's order: the problem's cost goals, then the
    solver's multiplier term.  Per-point inputs: states, controls,
    accelerations, auxiliary derivatives, multipliers (slacks last; no goal
    reads them)."""
    NS, NC = nlp.NS, nlp.NC
    sidx = {n: i for i, n in enumerate(rep.state_names)}
    cidx = {n: i for i, n in enumerate(rep.control_names)}
    out = []
    for g in st.problem.goals:
        if isinstance(g, MocoInitialActivationGoal):
            continue   # an endpoint constraint
        if isinstance(g, MocoControlGoal):
            tw = [(NS + cidx[n], float(g.control_weights.get(n, 1.0))) for n in rep.control_names]
            tw = [(i, w) for i, w in tw if w != 0.0]
            out.append(Goal("control", g.name, float(g.weight), np.array([i for i, _ in tw], int),
                            np.array([w for _, w in tw], float), exponent=int(g.exponent)))
        elif isinstance(g, MocoSumSquaredStateGoal):
            tw = [(sidx[n], float(g.state_weights.get(n, 1.0))) for n in rep.state_names]
            tw = [(i, w) for i, w in tw if w != 0.0]
            out.append(Goal("sum_squared_state", g.name, float(g.weight), np.array([i for i, _ in tw], int),
                            np.array([w for _, w in tw], float)))
        elif isinstance(g, MocoStateTrackingGoal):
            tab = Table(rep, g.reference.name)
            out.append(Goal("state_tracking", g.name, float(g.weight),
                            np.array([sidx[n] for n in tab.columns], int),
                            np.array([float(g.state_weights.get(n, 1.0)) for n in tab.columns], float),
                            table=tab, cols=np.arange(len(tab.columns))))
        elif isinstance(g, ImplicitAuxiliaryDerivativesTerm):
            out.append(Goal("aux_derivatives", g.name, float(g.weight),
                            NS + NC + nlp.NACC + np.arange(nlp.NAR), np.ones(nlp.NAR)))
        elif isinstance(g, MocoFinalTimeGoal):
            out.append(Goal("final_time", g.name, float(g.weight)))
        elif isinstance(g, MocoMarkerFinalGoal):
            mk = st.problem.model.markers[g.point_name]
            out.append(Goal("marker_final", g.name, float(g.weight),
                            marker=(mk.body, tuple(float(v) for v in mk.location),
                                    tuple(float(v) for v in g.reference_location))))
        else:
            raise TypeError(f"no restatement of {type(g).__name__} here")
    if st.solver.minimize_lagrange_multipliers:
        W = float(st.solver.lagrange_multiplier_weight) or 1.0
        out.append(Goal("multipliers", "lagrange_multipliers", W,
                        NS + NC + nlp.NDV + np.arange(nlp.NM), np.ones(nlp.NM)))
    return out


def quadrature(nlp, intervals=None):
    """(grid, weights over [0, 1]): the double mesh i / N and its midpoints,
    as the device holds them; the weights (Hermite-Simpson: 1/6, 2/3, 1/6 of
    each mesh interval; trapezoidal: 1/2, 1/2) in long double, over the mesh
    intervals ``intervals`` = (begin, end) only when given (a shard)."""
    g = _lanes.grid(nlp).astype(LD)
    N = nlp.opts.num_mesh_intervals
    a, b = intervals or (0, N)
    w = np.zeros(nlp.G, LD)
    one = LD(1)
    if nlp.opts.transcription == abi.MH_HERMITE_SIMPSON:
        for i in range(a, b):
            dm = g[2 * i + 2] - g[2 * i]
            w[2 * i] += dm / 6; w[2 * i + 1] += 2 * one * dm / 3; w[2 * i + 2] += dm / 6
    else:
        for i in range(a, b):
            dm = g[i + 1] - g[i]
            w[i] += dm / 2; w[i + 1] += dm / 2
    return g, w


def integrand(goal, P, t, TA):
    """(L, A) [G] of an integral goal at the double inputs P [G, NI] and
    times t [G].  TA [G]: the magnitudes that form t (|dur g| + |t0|); a
    tracking term's A carries |dL/dt| TA for the roundings of t itself."""
    G = P.shape[0]
    if goal.idx.size == 0:
        return np.zeros(G, LD), np.zeros(G, LD)
    V = P[:, goal.idx].astype(LD)
    w = goal.w.astype(LD)
    if goal.kind == "state_tracking":
        r, Ar, dr = goal.table.eval(goal.cols, t)
        d = V - r
        Ad = np.abs(V) + Ar
        L = (w * (d * d)).sum(1)
        A = (np.abs(w) * (d * d + 2 * np.abs(d) * (Ad + np.abs(dr) * TA[:, None]))).sum(1)
        return L, A
    if goal.kind == "control" and goal.exponent != 2:
        a = V if goal.signed else np.abs(V)
        term = a
        for _ in range(goal.exponent - 1):
            term = term * a
    else:
        term = V * V
    return (w * term).sum(1), (np.abs(w) * np.abs(term)).sum(1)


def roundings(goal, chain_bodies=0):
    """Roundings on the longest path of goal_integrand for this goal (of
    k_marker_final's cost for a marker goal), each at most eps / 2 of the
    magnitudes A sums."""
    T = int(goal.idx.size)           # L += term: the first term passes T adds
    if goal.kind == "control" and goal.exponent != 2:
        return 4 + 1 + T             # pow at 2 ulp = 4 half-ulps; w *
    if goal.kind in ("control", "sum_squared_state", "aux_derivatives", "multipliers"):
        return 2 + T                 # v * v; w *
    if goal.kind == "state_tracking":
        # on d: t = dur g + t0 (2), + h seed (2), dt = t - break (1), Horner
        # (2 per degree), s - r (1); then d * d (its factor 2 is in A), w *
        return 2 * goal.table.degree + 6 + 2 + T
    if goal.kind == "marker_final":
        # per chain body (joint_pose_stage): R_GF (3), axis_rot (sincos 4,
        # products 3), R_cur (3), R_GM (3), R_BM (3), the origin (5): 24; the
        # station (mv3 3, + p 1, - r 1); in double on both sides, hence twice;
        # then d * d and the three-term sum
        return 2 * (24 * chain_bodies + 5) + 2 + 3
    return 1                         # final time: W * tf


@dataclass
class Result:
    f: float
    A_f: float
    T_f: float
    terms: np.ndarray
    A_terms: np.ndarray
    K_terms: np.ndarray
    grad: np.ndarray
    A_grad: np.ndarray
    T_grad: np.ndarray
    zero: np.ndarray      # entries no goal reads: exactly 0.0 on the device
    kinds: List[str]


def _marker_cost(model, q, marker):
    """(cost, A): |p_G - r|^2 through the double-precision forward
    kinematics of test_frame_distance."""
    from test_frame_distance import forward_kinematics, station
    body, loc, ref = marker
    P, _ = station(model, forward_kinematics(model, q), body, loc, len(q))
    reach = float(np.linalg.norm(loc))
    parent = {j.child: j for j in model.joints}
    b, nb = body, 0
    while b != "ground":
        j = parent[b]
        reach += float(np.linalg.norm(j.loc_in_parent)) + float(np.linalg.norm(j.loc_in_child))
        b, nb = j.parent, nb + 1
    d = P.astype(LD) - np.array(ref, LD)
    Ad = reach + np.abs(np.array(ref, LD))
    return (d * d).sum(), (d * d + 2 * np.abs(d) * Ad).sum(), nb


def evaluate(nlp, goals, x, intervals=None) -> Result:
    """The objective, its per-goal terms and its gradient at x, with bounds;
    ``intervals`` = (begin, end): the partial of that shard (its own
    quadrature, the endpoint goals on the shard that holds the last
    interval)."""
    x = np.asarray(x, float)
    n, G, NI = nlp.n, nlp.G, nlp.NI
    N = nlp.opts.num_mesh_intervals
    ND = NI - nlp.NSL                 # the goal callback's inputs: no slacks
    endpoint = intervals is None or intervals[1] == N
    gd = _lanes.grid(nlp)
    gl, q = quadrature(nlp, intervals)
    fd = nlp.opts.finite_difference_scheme
    h = nlp.opts.fd_step if nlp.opts.fd_step > 0 else 1e-8
    hl = LD(h)
    den = 2 * hl if fd == abi.MH_FD_CENTRAL else hl
    P = nlp.point_inputs(x)
    cols = nlp.point_inputs(np.arange(n, dtype=float)).astype(np.int64)   # a pure gather
    t = (x[1] - x[0]) * gd + x[0]     # double, as the kernels form it
    dur = LD(x[1]) - LD(x[0])
    TA = np.abs(dur * gl) + abs(LD(x[0]))
    ng = len(goals)
    R = -(-G // 256) + 8              # k_reduce_obj: strided adds, then 8 tree levels
    terms, A_terms, K_terms = np.zeros(ng, LD), np.zeros(ng, LD), np.zeros(ng)
    grad, A_grad, T_grad = np.zeros(n, LD), np.zeros(n, LD), np.zeros(n, LD)
    zero = np.ones(n, bool)
    model = nlp.rep.problem.model

    def leg(goal, d, sign):
        if d < 2:
            seed = (1.0 - gd) if d == 0 else gd
            return integrand(goal, P, t + sign * h * seed, TA)
        Pp = P.copy()
        Pp[:, d - 2] = P[:, d - 2] + sign * h
        return integrand(goal, Pp, t, TA)

    for gi, goal in enumerate(goals):
        W = LD(goal.W)
        if goal.kind == "final_time":
            K_terms[gi] = 2 * roundings(goal)
            if endpoint:
                terms[gi], A_terms[gi] = W * LD(x[1]), abs(W * LD(x[1]))
                grad[1] += W           # exact: g1 += G.weight
                zero[1] = False
            continue
        if goal.kind == "marker_final":
            qf = P[G - 1, :nlp.NQ].copy()
            c0, A0, nb = _marker_cost(model, qf, goal.marker)
            c = roundings(goal, nb)
            K_terms[gi] = 2 * (c + 1)
            if not endpoint:
                continue
            terms[gi], A_terms[gi] = W * c0, abs(W) * A0
            for s in range(nlp.NQ):
                cp = cm = (c0, A0)
                if fd != abi.MH_FD_BACKWARD:
                    qq = qf.copy(); qq[s] = qf[s] + h
                    cp = _marker_cost(model, qq, goal.marker)[:2]
                if fd != abi.MH_FD_FORWARD:
                    qq = qf.copy(); qq[s] = qf[s] - h
                    cm = _marker_cost(model, qq, goal.marker)[:2]
                col = cols[G - 1, s]
                a = abs(W) * (cp[1] + cm[1]) / den
                grad[col] += W * ((cp[0] - cm[0]) / den)
                A_grad[col] += a
                T_grad[col] += 2 * (c + 4) * a    # -, / h, W *, += onto k_grad's entry
                zero[col] = False
            continue
        c = roundings(goal)
        # quad[k] (1/6 rounded, * dm, the += of two intervals: 3), quad * L,
        # the reduction, x1 - x0, dur * acc, W *
        K_terms[gi] = 2 * (c + 3 + 1 + R + 3)
        L0, A0 = integrand(goal, P, t, TA)
        acc, A_acc = (q * L0).sum(), (q * A0).sum()
        terms[gi], A_terms[gi] = W * (dur * acc), abs(W * dur) * A_acc
        if goal.idx.size == 0:
            continue
        wq = W * dur * q
        # both legs (c each), -, / h; x1 - x0, W * dur, quad (3), * quad, * dL; the goal sum
        Kg = 2 * (c + 2 + 7 + ng)
        for d in range(ND + 2):
            if goal.kind == "multipliers":
                j = d - 2 - (nlp.NS + nlp.NC + nlp.NDV)
                if d < 2 or j < 0 or j >= nlp.NM:
                    continue
                dL = LD(goal.w[j]) * (2 * P[:, d - 2].astype(LD))     # exact: w 2 lambda
                AdL, Kd = np.abs(dL), 2 * (1 + 7 + ng)
            else:
                lp = leg(goal, d, +1.0) if fd != abi.MH_FD_BACKWARD else (L0, A0)
                lm = leg(goal, d, -1.0) if fd != abi.MH_FD_FORWARD else (L0, A0)
                dL, AdL, Kd = (lp[0] - lm[0]) / den, (lp[1] + lm[1]) / den, Kg
            val, a = wq * dL, np.abs(wq) * AdL
            if d < 2:
                grad[d] += val.sum(); A_grad[d] += a.sum()
                T_grad[d] += (Kd + 2 * (R + 1)) * a.sum()   # the reduction of tpart, + g0 / g1
            else:
                grad[cols[:, d - 2]] += val
                A_grad[cols[:, d - 2]] += a
                T_grad[cols[:, d - 2]] += Kd * a
        # d/dt0 and d/dtf of the duration factor: -+ W acc, summed over the goals
        for d, s in ((0, -1), (1, 1)):
            grad[d] += s * W * acc
            A_grad[d] += abs(W) * A_acc
            T_grad[d] += 2 * (c + 3 + 1 + R + 1 + ng + 1) * abs(W) * A_acc
        zero[:2] = False
        zero[cols[:, goal.idx].ravel()] = False
    f, A_f = terms.sum(), A_terms.sum()
    T_f = (K_terms * A_terms).sum() + 2 * ng * A_f    # total += term
    return Result(f, A_f, T_f, terms, A_terms, K_terms, grad, A_grad, T_grad, zero,
                  [g.kind for g in goals])


def ratios(res: Result, f=None, terms=None, grad=None):
    """max |value - reference| / (eps A) per compared thing (0 / 0 = 0),
    and whether each is within eps T."""
    out = {}

    def one(name, v, ref, A, T):
        err = np.abs(np.asarray(v, float).astype(LD) - ref)
        r = np.where(A > 0, err / np.where(A > 0, EPS * A, 1), np.where(err > 0, np.inf, 0))
        out[name] = (float(np.max(r, initial=0.0)), bool(np.all(err <= EPS * T)))
    if f is not None:
        one("f", [f], np.array([res.f]), np.array([res.A_f]), np.array([res.T_f]))
    if terms is not None:
        one("terms", terms, res.terms, res.A_terms, res.K_terms * res.A_terms)
    if grad is not None:
        one("grad", grad, res.grad, res.A_grad, res.T_grad)
    return out
