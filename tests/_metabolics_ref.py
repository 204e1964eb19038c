"""The checker of test_metabolics.py: a NumPy restatement of
Bhargava2004Metabolics::calcMetabolicRate (Bhargava2004Metabolics.cpp:337-537),
its three conditionals (177-215), the muscle mass (40-50), the basal rate
(217-225) and the fibre-length dependence curve (78-82), written from the
definitions in include/mocohip.h.  It reads a muscle's quantities from
test_muscle_outputs.restated_outputs and calls no library code under test; the
component's options and a muscle's parameters are read as plain attributes.
``real`` = numpy.longdouble evaluates the model (not the muscle) in extended
precision."""
import math

import numpy as np

EPS_V = 1e-16   # added to the fibre velocity, as the reference does


def conditional(mode, cond, left, right, k, direction, real=float):
    """left where cond <= 0, right where cond > 0: mode "none" (a step), "tanh"
    or "huber" (smoothing k; direction +1 / -1: the side the ramp rises on)."""
    cond, left, right, k = real(cond), real(left), real(right), real(k)
    if mode == "none":
        return left if cond <= 0 else right
    if mode == "tanh":
        return left + (-left + right) * (real(0.5) + real(0.5) * np.tanh(k * cond))
    assert mode == "huber"
    offset = left if direction == 1 else right
    scale = (right - left) / cond
    state = direction * cond
    y = k * (state + real(0.5) * (1 / k))
    if y < 0:
        f = offset
    elif y <= 1:
        f = real(0.5) * y * y + offset
    else:
        f = (y - real(0.5)) + offset
    return scale * (f / k + offset * (1 - 1 / k))


def length_dependence(nfl, real=float):
    """The piecewise-linear curve through (0, .5) (.5, .5) (1, 1) (1.5, 0) (10, 0)."""
    return real(np.interp(float(nfl), [0.0, 0.5, 1.0, 1.5, 10.0], [0.5, 0.5, 1.0, 0.0, 0.0])) if real is float else \
        _interp_exact(real(nfl), real)


def _interp_exact(x, real):
    xs, ys = [0.0, 0.5, 1.0, 1.5, 10.0], [0.5, 0.5, 1.0, 0.0, 0.0]
    for i in range(4):
        if x <= xs[i + 1]:
            return real(ys[i]) + (real(ys[i + 1]) - real(ys[i])) * (x - real(xs[i])) / (real(xs[i + 1]) - real(xs[i]))
    return real(0.0)


def mode_of(comp):
    return comp.smoothing_type if comp.use_smoothing else "none"


def muscle_mass(mp, muscle):
    """The provided mass, or Fmax / specific tension * density * optimal fibre length."""
    if not math.isnan(mp.muscle_mass):
        return mp.muscle_mass
    return muscle.max_isometric_force / mp.specific_tension * mp.density * muscle.optimal_fiber_length


def muscle_rates(comp, mp, mass, Fmax, q, real=float):
    """The rates of one muscle from q = its outputs by name (activation,
    excitation, active_fiber_force, passive_fiber_force,
    normalized_fiber_length, fiber_velocity, active_force_length_multiplier):
    a dict with activation, maintenance, shortening, work, total, and the two
    quantities the clamps switch on: ``power`` (the sum before the power
    clamp) and ``heat`` (the total heat before the minimum)."""
    mode = mode_of(comp)
    tanh_mode = "none" if mode == "none" else "tanh"
    s = real(comp.muscle_effort_scaling_factor)
    act, exc = s * real(q["activation"]), s * real(q["excitation"])
    Fp, Fa = real(q["passive_fiber_force"]), s * real(q["active_fiber_force"])
    Ft = Fa + Fp
    v = real(q["fiber_velocity"])
    r = real(mp.ratio_slow_twitch_fibers)
    half_pi = real(np.pi) / 2 if real is not float else math.pi / 2
    slow = r * np.sin(half_pi * exc)
    fast = (1 - r) * (1 - np.cos(half_pi * exc))
    Fiso = act * real(q["active_force_length_multiplier"]) * real(Fmax)
    m = real(mass)
    A = m * (real(mp.activation_constant_slow_twitch) * slow + real(mp.activation_constant_fast_twitch) * fast)
    M = m * length_dependence(q["normalized_fiber_length"], real) * (
        real(mp.maintenance_constant_slow_twitch) * slow + real(mp.maintenance_constant_fast_twitch) * fast)
    ve = v + real(EPS_V)
    kv, kp, kh = comp.velocity_smoothing, comp.power_smoothing, comp.heat_rate_smoothing
    if comp.use_force_dependent_shortening_prop_constant:
        alpha = conditional(tanh_mode, ve, real(0.16) * Fiso + real(0.18) * Ft, real(0.157) * Ft, kv, -1, real)
    else:
        alpha = conditional(mode, ve, real(0.25) * Ft, 0.0, kv, -1, real)
    S = -alpha * ve
    if comp.include_negative_mechanical_work:
        W = -Fa * v
    else:
        W = conditional(mode, ve, -Fa * v, 0.0, kv, -1, real)
    power = A + M + S + W
    if comp.forbid_negative_total_power:
        if mode != "none":
            S = S - conditional(mode, -power, 0.0, power, kp, 1, real)
        elif power < 0:
            S = S - power
    heat = A + M + S
    H = heat
    if comp.enforce_minimum_heat_rate_per_muscle:
        if mode != "none":
            H = conditional(mode, -heat + m, heat, m, kh, 1, real)
        elif heat < m:
            H = m
    return {"activation": A, "maintenance": M, "shortening": S, "work": W, "total": H + W, "power": power,
            "heat": heat}


def basal_rate(comp, model):
    return comp.basal_coefficient * sum(float(b.mass) for b in model.bodies.values()) ** comp.basal_exponent


def model_muscle(model, mp):
    return next(i for i, mu in enumerate(model.muscles) if mp.muscle_path in (mu.path, mu.name))


def component_rates(comp, ck, row, real=float):
    """Every muscle's rates at one row [t, point inputs], in the component's
    order (ck: test_muscle_outputs.Checker)."""
    from test_muscle_outputs import NAMES
    out = []
    for mp in comp.muscles:
        im = model_muscle(ck.model, mp)
        mu = ck.model.muscles[im]
        q = dict(zip(NAMES, ck.outputs(im, row)))
        out.append(muscle_rates(comp, mp, muscle_mass(mp, mu), mu.max_isometric_force, q, real))
    return out


def component_outputs(comp, ck, row, real=float):
    """[total metabolic rate (with the basal rate), total activation,
    maintenance, shortening and work rates, then each muscle's metabolic
    rate]: mh_eval_metabolics' row."""
    rates = component_rates(comp, ck, row, real)
    tot = [sum((r[k] for r in rates), real(0.0)) for k in ("total", "activation", "maintenance", "shortening", "work")]
    tot[0] = tot[0] + real(basal_rate(comp, ck.model))
    return np.array(tot + [r["total"] for r in rates], dtype=real)
