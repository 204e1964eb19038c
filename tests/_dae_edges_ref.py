"""The DAE's building blocks (csrc/dae_device.hpp: the DeGrooteFregly2016
curves and muscle, the SimmSpline evaluators, the piecewise-polynomial tables)
restated in numpy.longdouble from the Python Model / ProblemRep alone (test
helper: no tests here, no call into the oracle or the library).

Every quantity is a ``B``: a long-double value v with an absolute bound e on
what the device's double arithmetic may differ from it by.  The bound follows
the device source operation by operation, to first order:

    a +- b      e_a + e_b + eps |v|
    a * b       |a| e_b + |b| e_a + eps |v|
    a / b       (e_a + |v| e_b) / |b| + eps |v|
    f(u)        |f'(u)| e_u + U eps |v|
    an input    0

with eps = 2^-52 (twice the half-ulp of a correctly rounded operation: the
margin of _objective_ref) and U the limit the OpenCL specification gives for
the double-precision library function, which ROCm's device library states it
meets: sqrt 1 (correctly rounded), exp 3, log 3, sinh 4, tanh 5, asin 4.  A
multiplication by a literal (2.0 *, 0.5 *) counts like any other; a fused
multiply-add only removes a rounding.  A test asserts |device - v| <= e."""
import math

import numpy as np

from _objective_ref import EPS, LD
from mocohip import abi
from mocohip.splines import SimmSpline

NAMES = abi.MUSCLE_OUTPUTS


class B:
    """A long-double value (array or scalar) with its absolute bound."""
    __slots__ = ("v", "e")
    __array_ufunc__ = None   # ndarray op B defers to B's reflected operator

    def __init__(self, v, e=None):
        self.v = np.asarray(v, LD)
        self.e = np.zeros_like(self.v) if e is None else np.broadcast_to(np.asarray(e, LD), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, B) else B(np.asarray(x, float))   # a double: an input, exact

    def __neg__(self):
        return B(-self.v, self.e)

    def __add__(self, o):
        o = B.of(o)
        v = self.v + o.v
        return B(v, self.e + o.e + EPS * np.abs(v))

    def __sub__(self, o):
        return self + (-B.of(o))

    def __rsub__(self, o):
        return B.of(o) + (-self)

    __radd__ = __add__

    def __mul__(self, o):
        o = B.of(o)
        v = self.v * o.v
        return B(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + EPS * np.abs(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = B.of(o)
        v = self.v / o.v
        return B(v, (self.e + np.abs(v) * o.e) / np.abs(o.v) + EPS * np.abs(v))

    def __rtruediv__(self, o):
        return B.of(o) / self

    def fn(self, f, df, U):
        v = f(self.v)
        return B(v, np.abs(df(self.v)) * self.e + U * EPS * np.abs(v))

    def sqrt(self):
        return self.fn(np.sqrt, lambda u: 1 / (2 * np.sqrt(u)), 1)

    def exp(self):
        return self.fn(np.exp, np.exp, 3)

    def log(self):
        return self.fn(np.log, lambda u: 1 / u, 3)

    def sinh(self):
        return self.fn(np.sinh, np.cosh, 4)

    def tanh(self):
        return self.fn(np.tanh, lambda u: 1 - np.tanh(u) ** 2, 5)

    def asin(self):
        return self.fn(np.arcsin, lambda u: 1 / np.sqrt(1 - u * u), 4)


def ratio(got, want: B):
    """|got - v| / e entry by entry; 0 / 0 = 0, anything / 0 = inf."""
    err = np.abs(np.asarray(got, float).astype(LD) - want.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(want.e > 0, err / np.where(want.e > 0, want.e, 1), np.where(err > 0, np.inf, 0))
    return r.astype(float)


# ---- the muscle -------------------------------------------------------------------

# DeGrooteFregly2016Muscle.h:769-817 as csrc/dae_device.hpp:270-277 spells them
FAL = [[0.8150671134243542, 1.055033428970575, 0.162384573599574, 0.063303448465465],
       [0.433004984392647, 0.716775413397760, -0.029947116970696, 0.200356847296188],
       [0.1, 1.0, 0.353553390593274, 0.0]]
D1, D2, D3, D4 = -0.3211346127989808, -8.149, -0.374, 0.8825327733249912
C1, C2, C3 = 0.2, 1.0, 0.2
INV_C1 = 1.0 / C1      # literals the compiler folds in double: data
INV_D1 = 1.0 / D1


def derived_formulas(mu, T=float):
    """The six constants of mus_derived by csrc/mocohip.hip:2496-2502, every
    operand a double, the arithmetic in type T (float: as the host forms them)."""
    sin, log, exp = (math.sin, math.log, math.exp) if T is float else (np.sin, np.log, np.exp)
    lopt, alpha = T(mu.optimal_fiber_length), T(mu.pennation_angle_at_optimal)
    d0 = lopt * sin(alpha)
    d4 = exp(T(4.0) * (T(0.2) - T(1.0)) / T(mu.passive_fiber_strain_at_one_norm_force))
    return [d0, d0 * d0, T(mu.max_contraction_velocity) * lopt,
            log((T(1.0) + T(0.2)) / T(0.2)) / (T(1.0) + T(mu.tendon_strain_at_one_norm_force) - T(1.0)),
            d4, exp(T(4.0)) - d4]


class Muscle:
    """One muscle's data: its C struct's fields and the derived constants in
    double (data here: the device reads them from mus_derived)."""

    def __init__(self, rep, im=0):
        mu = rep.compiled._muscles[im]
        self.mu = mu
        self.derived = [float(v) for v in derived_formulas(mu, float)]
        self.rigid = bool(mu.ignore_tendon_compliance)
        self.implicit_tendon = (not self.rigid) and bool(mu.tendon_dynamics_implicit)
        self.has_act = not bool(mu.ignore_activation_dynamics)
        self.passive = not bool(mu.ignore_passive_fiber_force)


def gauss_like(x, b1, b2, b3, b4):
    """dae_device.hpp:263-267"""
    num = (x - b2) * (x - b2)
    den = (b3 + b4 * x) * (b3 + b4 * x)
    return b1 * (-0.5 * num / den).exp()


def dgf_fal(scale, l, consts=FAL):
    """dae_device.hpp:268-275"""
    x = (l - 1.0) / scale + 1.0
    return gauss_like(x, *consts[0]) + gauss_like(x, *consts[1]) + gauss_like(x, *consts[2])


def dgf_fv(v):
    """dae_device.hpp:278-282"""
    tv = D2 * v + D3
    arg = tv + (tv * tv + 1.0).sqrt()
    return D1 * arg.log() + D4


def fv_inv_argument(fv):
    return INV_D1 * (fv - D4)


def dgf_fv_inv(fv, omit_d3=False):
    """dae_device.hpp:283-285"""
    s = fv_inv_argument(fv).sinh()
    return (s if omit_d3 else s - D3) / D2


def dgf_fpe(M, nfl, no_offset=False):
    """dae_device.hpp:322-325, 391-394"""
    ex = (4.0 * (nfl - 1.0) / M.mu.passive_fiber_strain_at_one_norm_force).exp()
    return (ex if no_offset else ex - M.derived[4]) / M.derived[5]


def tendon_length(M, ftn):
    """The normalized tendon length of dae_device.hpp:315, :383"""
    return (INV_C1 * (B.of(ftn) + C3)).log() / M.derived[3] + C2


def muscle(M: Muscle, L, S, act, exc, ftn, dft, mutation=None):
    """dgf_outputs / dgf_output (dae_device.hpp:374-471) and dgf_eval / dgf_adot
    (:291-357), which share their expressions: a dict of B, the 34 outputs by
    name plus what the DAE takes, "adot", "ftdot", "residual", and the
    argument of sinh, "sinh_argument".  L, S: B; the rest doubles.  A muscle
    without activation dynamics runs on its excitation (dae_eval:1044)."""
    mu = M.mu
    fiberWidth, sqW, vmax, kT, peOffset, peDenom = M.derived
    lopt, lts, Fmax = mu.optimal_fiber_length, mu.tendon_slack_length, mu.max_isometric_force
    compliant = not M.rigid
    L, S = B.of(L), B.of(S)
    exc = B.of(exc)
    act = B.of(act) if M.has_act else exc
    ftn, dft = B.of(ftn), B.of(dft)
    zero = B(np.zeros(L.v.shape))
    nTL = tendon_length(M, ftn) if compliant else B(np.ones(L.v.shape))
    tendonStrain = nTL - 1.0
    tendonLength = lts * nTL
    flat = L - tendonLength
    fiberLength = (flat * flat + sqW).sqrt()
    nfl = fiberLength / lopt
    cosPenn = flat / fiberLength
    fPE = dgf_fpe(M, nfl, mutation == "no_passive_offset") if M.passive else zero
    consts = FAL
    if mutation == "fal_constant":
        consts = [list(r) for r in FAL]
        consts[0][1] *= 1.0 + 1e-9
    fAL = dgf_fal(mu.active_force_width_scale, nfl, consts)
    sinh_arg = zero
    if compliant and not M.implicit_tendon:
        nff = ftn / cosPenn
        fV = (nff - fPE) / (act * fAL)
        sinh_arg = fv_inv_argument(fV)
        nfv = dgf_fv_inv(fV, mutation == "no_d3")
        fiberVelocity = nfv * vmax
        fvat = fiberVelocity / cosPenn
        tendonVelocity = S - fvat
        ntv = tendonVelocity / lts
    else:
        ntv = dft / (C1 * kT * (kT * (nTL - C2)).exp()) if compliant else zero
        tendonVelocity = lts * ntv
        fvat = S - tendonVelocity
        fiberVelocity = fvat * cosPenn
        nfv = fiberVelocity / vmax
        fV = dgf_fv(nfv)
    activeF = Fmax * (act * fAL * fV)
    conPass = Fmax * fPE
    nonCon = Fmax * mu.fiber_damping * nfv
    total = activeF + conPass + nonCon
    passiveF = conPass + nonCon
    T = Fmax * ftn if compliant else total * cosPenn
    out = {"length": L, "lengthening_speed": S, "activation": act, "excitation": exc, "fiber_length": fiberLength,
           "normalized_fiber_length": nfl, "pennation_angle": (fiberWidth / fiberLength).asin(),
           "cos_pennation_angle": cosPenn, "tendon_length": tendonLength, "tendon_strain": tendonStrain,
           "fiber_length_along_tendon": flat, "active_force_length_multiplier": fAL,
           "passive_force_multiplier": fPE, "fiber_velocity": fiberVelocity, "normalized_fiber_velocity": nfv,
           "fiber_velocity_along_tendon": fvat, "tendon_velocity": tendonVelocity,
           "force_velocity_multiplier": fV,
           "pennation_angular_velocity": -fiberVelocity / fiberLength * (fiberWidth / flat),
           "fiber_force": total, "fiber_force_along_tendon": total * cosPenn, "active_fiber_force": activeF,
           "passive_fiber_force": passiveF, "active_fiber_force_along_tendon": activeF * cosPenn,
           "passive_fiber_force_along_tendon": passiveF * cosPenn, "tendon_force": T,
           "passive_fiber_elastic_force": conPass, "passive_fiber_elastic_force_along_tendon": conPass * cosPenn,
           "passive_fiber_damping_force": nonCon, "passive_fiber_damping_force_along_tendon": nonCon * cosPenn,
           "fiber_active_power": -(activeF + nonCon) * fiberVelocity, "fiber_passive_power": -conPass * fiberVelocity,
           "tendon_power": -T * tendonVelocity, "muscle_power": -T * S}
    assert list(out) == list(NAMES)
    out["sinh_argument"] = sinh_arg
    if M.has_act:   # dgf_adot, dae_device.hpp:291-299
        tcf = 0.5 + 1.5 * act
        tempAct = 1.0 / (mu.activation_time_constant * tcf)
        tempDeact = tcf / mu.deactivation_time_constant
        f = 0.5 * (0.1 * (exc - act)).tanh()
        timeConst = tempAct * (f + 0.5) + tempDeact * (-f + 0.5)
        out["adot"] = timeConst * (exc - act)
    if compliant:
        out["ftdot"] = dft if M.implicit_tendon else ntv * (C1 * kT * (kT * (nTL - C2)).exp())
    if M.implicit_tendon:
        out["residual"] = T - total * cosPenn
    return out


def slider_path(q, u):
    """The straight two-point path along the slider's axis by dae_eval's
    length / speed loop (dae_device.hpp:1033-1041, mo_device.hpp:181-191): d =
    (q, 0, 0) and e = (u, 0, 0), so L = sqrt(q q) = |q| (exact: the square
    root of a rounded square is the number) and S = (q u) / |q| (a product and
    a quotient)."""
    q, u = B.of(q), B.of(u)
    return B(np.abs(q.v), q.e), q * u / B(np.abs(q.v), q.e)


def slider_udot(m, g, T, q):
    """dae_eval on the slider with explicit dynamics: the body force m (-g)
    (dae_device.hpp:946-950), the tension as a point force T d0 / l at the body
    (:1058, :1081), tau = -S . F (:1136), the 1 x 1 Cholesky factor sqrt(m) and
    its two solves (:1194-1211)."""
    q = B.of(q)
    F = B.of(m) * (-g) + T * q / B(np.abs(q.v), q.e)
    d = B.of(m).sqrt()
    return (-F) / d / d


def slider_residual(m, g, T, q, udot):
    """dae_eval with prescribed kinematics on the slider: A = -g + udot
    (:873-877), F = m A + T d0 / l, the residual S . F (:1136-1138)."""
    q = B.of(q)
    return B.of(m) * (udot + (-g)) + T * q / B(np.abs(q.v), q.e)


# ---- SimmSpline -------------------------------------------------------------------

class Spline:
    """A compiled SimmSpline function: its knots, and the coefficients the
    host forms in double (splines.SimmSpline: mocohip.hip simm_coefficients'
    restatement), which are data here."""

    def __init__(self, rep, fi):
        ms = rep.compiled.struct
        F = ms.functions[fi]
        assert F.kind == abi.MH_FN_SIMMSPLINE
        n, kb = int(F.knot_count), int(F.knot_begin)
        self.x = np.array([ms.knot_x[kb + i] for i in range(n)], float)
        self.y = np.array([ms.knot_y[kb + i] for i in range(n)], float)
        s = SimmSpline(self.x, self.y)
        self.b, self.c, self.d = s.b.copy(), s.c.copy(), s.d.copy()
        self.n, self.scale, self.coord = n, float(F.scale), int(F.coord)

    def segments(self, t):
        """The admissible expansion points of simm_eval / simm_eval_n /
        simm_eval_k (dae_device.hpp:167-194, :1223-1243, :1319-1333) at a t
        inside the knot range: the segment that holds t; at an interior knot
        either neighbour; in the 2e-13 window of the first knot segment 0; in
        the window of the last knot the expansion about it or its neighbour."""
        x, n = self.x, self.n
        if abs(t - x[0]) <= 2e-13:
            return [0]
        if abs(t - x[n - 1]) <= 2e-13:
            return [n - 1, n - 2]
        k = int(np.searchsorted(x, t, side="right")) - 1
        return [k - 1, k] if t == x[k] and k > 0 else [k]

    def eval(self, t, mutation=None):
        """[(value, first, second derivative)] as B, one per admissible
        expansion; outside the range the linear extrapolation, its second
        derivative exactly 0."""
        x, y, b, c, d, n = self.x, self.y, self.b, self.c, self.d, self.n
        t = float(t)
        if n == 1:
            return [(B(y[0]), B(0.0), B(0.0))]
        for end, nb in ((0, 1), (n - 1, n - 2)):
            if (t < x[0]) if end == 0 else (t > x[n - 1]):
                slope = b[nb] if mutation == "neighbour_slope" else b[end]
                return [(y[end] + (B.of(t) - x[end]) * slope, B(slope), B(0.0))]
        out = []
        for k in self.segments(t):
            dx = B.of(t) - x[k]
            out.append((y[k] + dx * (b[k] + dx * (c[k] + dx * d[k])),
                        b[k] + dx * (2.0 * c[k] + 3.0 * dx * d[k]),
                        2.0 * c[k] + 6.0 * dx * d[k]))
        return out


def coupler_outputs(K_scale, sp, q_i, q_d, u_i, u_d, a_i, a_d, gam):
    """kc_outputs (dae_device.hpp:791-817) of one CoordinateCoupler with the
    derivatives enforced: per admissible spline expansion the B's [position,
    velocity, acceleration error, velocity correction of the independent and
    of the dependent coordinate]; fn_eval's scale (:210) first."""
    res = []
    for v, d1, d2 in sp:
        v, d1, d2 = v * K_scale[1], d1 * K_scale[1], d2 * K_scale[1]
        gi = K_scale[0] * d1
        res.append([K_scale[0] * v - q_d, gi * u_i - u_d,
                    (gi * a_i - a_d) + K_scale[0] * d2 * u_i * u_i, gi * gam, -B.of(gam)])
    return res


# ---- tables -------------------------------------------------------------------------

class Table:
    """A compiled table: breaks and coefficients in t - break, lowest order
    first, both data."""

    def __init__(self, rep, name):
        ms = rep.compiled.struct
        T = ms.tables[rep.compiled.table_index[name]]
        self.columns = list(rep.compiled.table_columns[name])
        self.nseg, self.ncol, self.degree = int(T.nseg), int(T.ncol), int(T.degree)
        self.br = np.array([ms.table_breaks[T.break_begin + i] for i in range(self.nseg + 1)], float)
        n = self.degree + 1
        cf = [ms.table_coefs[T.coef_begin + i] for i in range(self.nseg * self.ncol * n)]
        self.cf = np.array(cf, float).reshape(self.nseg, self.ncol, n)

    def segment(self, t, mutation=None):
        """The last segment whose break is <= t; segment 0 for t <= br[0], the
        last for t >= br[nseg] (table_eval_d, dae_device.hpp:215-229)."""
        t = np.asarray(t, float)
        side = "left" if mutation == "old_segment" else "right"
        s = np.searchsorted(self.br, t, side=side) - 1
        s = np.where(t <= self.br[0], 0, s)
        return np.where(t >= self.br[-1], self.nseg - 1, s)

    def eval(self, col, t, mutation=None):
        """(value, first, second derivative) of column col at the double
        times t [R], by table_eval_d's Horner (dae_device.hpp:230-238)."""
        t = np.asarray(t, float)
        s = self.segment(t, mutation)
        dt = B.of(t) - self.br[s]
        c = self.cf[s, col, :]
        p, dp, ddp = B(c[:, self.degree]), B(np.zeros(t.shape)), B(np.zeros(t.shape))
        for k in range(self.degree - 1, -1, -1):
            ddp = ddp * dt + 2.0 * dp
            dp = dp * dt + p
            p = p * dt + c[:, k]
        return p, dp, ddp
