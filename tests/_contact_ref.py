"""numpy.longdouble restatement of the three station-plane contact force laws,
written from the reference's Moco/Moco/Components/StationPlaneContactForce.h
(calcContactForceOnStation of AckermannVanDenBogert2010Force,
EspositoMiller2018Force and MeyerFregly2016Force).  Calls no library code.

One deliberate difference: MeyerFregly2016's spring force is 0 where
(y + h) / c > 710.4758600739439, the overflow threshold of double cosh, which
the reference turns into "NaN or Inf -> 0"; long double does not overflow
there.  Test rows keep out of 709.7 < (y + h) / c < 710.5, where a device cosh
may overflow early."""
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is not wider than double here"

COSH_OVERFLOW = 710.4758600739439
MF_BAND = (709.7, 710.5)
MF_H, MF_C = 1e-3, 5e-4


def in_mf_band(y):
    z = (float(y) + MF_H) / MF_C
    return MF_BAND[0] < z < MF_BAND[1]


def avdb(f, y, vy, vx):
    y, vy, vx = LD(y), LD(vy), LD(vx)
    a, b = LD(f.stiffness), LD(f.dissipation)
    depth, depth_rate = LD(0) - y, LD(0) - vy
    fy = LD(0)
    if depth > 0:
        fy = max(LD(0), a * depth ** 3 * (1 + b * depth_rate))
    fy = fy + LD(1.0) * depth
    transition = np.tanh(vx / LD(f.tangent_velocity_scaling_factor) / 2)
    return -transition * LD(f.friction_coefficient) * fy, fy


def esposito_miller(f, y, vy, vx):
    y, vy, vx = LD(y), LD(vy), LD(vx)
    a, b = LD(f.stiffness), LD(f.dissipation)
    depth, depth_rate = LD(0) - y, LD(0) - vy
    d0sq = LD(f.depth_offset) * LD(f.depth_offset)
    dy = LD(0.5) * (np.sqrt(depth * depth + d0sq) + depth)
    fy = a * dy * dy * (1 + b * depth_rate) + LD(1.0) * depth
    transition = np.tanh(vx / LD(f.tangent_velocity_scaling_factor))
    return -transition * LD(f.friction_coefficient) * fy, fy


def meyer_fregly(f, y, vy, vx):
    y, vy, vx = LD(y), LD(vy), LD(vx)
    K, Cv, tscale = LD(f.stiffness), LD(f.dissipation), LD(f.tscale)
    depth_rate = LD(0) - vy
    klow = LD(1e-1) / (tscale * tscale)
    h, c, ymax = LD(MF_H), LD(MF_C), LD(1e-2)
    vp = (K + klow) / (K - klow)
    sp = (K - klow) / 2
    constant = -sp * (vp * ymax - c * np.log(np.cosh((ymax + h) / c)))
    if (y + h) / c > LD(COSH_OVERFLOW):
        spring = LD(0)
    else:
        spring = -sp * (vp * y - c * np.log(np.cosh((y + h) / c))) - constant
        if np.isnan(spring) or np.isinf(spring):
            spring = LD(0)
    fy = spring * (1 + Cv * depth_rate)
    mu = LD(1) * np.tanh(vx / LD(0.05) / 2)
    return -fy * mu, fy


LAWS = {"AckermannVanDenBogert2010Force": avdb, "EspositoMiller2018Force": esposito_miller,
        "MeyerFregly2016Force": meyer_fregly}


def force(f, y, vy, vx):
    """(fx, fy) in long double of contact force object ``f`` (its class name
    picks the law; its attributes are the reference's properties) at station
    height y, normal velocity vy and sliding velocity vx."""
    return LAWS[type(f).__name__](f, y, vy, vx)


def forces(f, rows):
    """[len(rows), 2] long double: force() at rows of (y, vy, vx)."""
    return np.array([force(f, *r) for r in rows], dtype=LD)
