// contact_device.hpp -- station-plane ground contact (the reference's
// Moco/Moco/Components/StationPlaneContactForce.h): a body-fixed station
// against the ground plane y = 0, friction along ground x only.  One force
// law, shared by dae_eval (dae_device.hpp) and k_contact_forces (contact.hip).
// A contact travels as an mh_external_force record of kind 1..3 whose
// force_col is the offset into mh_model.table_coefs of MH_CONTACT_PARAMS
// doubles (include/mocohip.h).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/mocohip.h"

namespace mh {

// The force on the body at the station, in ground (fz = 0), from the
// station's height y, normal velocity vy and sliding velocity vx (the
// ground-x component): the three calcContactForceOnStation bodies, operation
// for operation, each rounded on its own.  One deviation: AVDB's
// pow(depth, 3) is depth * depth * depth (no pow() in the interpreter; the two
// differ by a rounding).  p: station location (3), stiffness, dissipation,
// friction coefficient, tangent velocity scaling factor, depth_offset (EM) /
// tscale (MF).
__device__ __forceinline__ void contact_force(int kind, const double* __restrict__ p, double y, double vy,
        double vx, double& fx, double& fy) {
#pragma clang fp contract(off)
    const double stiffness = p[3], dissipation = p[4];
    const double depthRate = 0.0 - vy;
    if (kind == MH_EXT_CONTACT_MEYER_FREGLY) {
        const double tscale = p[7];
        const double klow = 1e-1 / (tscale * tscale);
        const double h = 1e-3, c = 5e-4, ymax = 1e-2;
        const double vp = (stiffness + klow) / (stiffness - klow);
        const double sp = (stiffness - klow) / 2;
        const double constant = -sp * (vp * ymax - c * log(cosh((ymax + h) / c)));
        double Fspring = -sp * (vp * y - c * log(cosh((y + h) / c))) - constant;
        // NaN or Inf (cosh overflows once (y + h) / c passes about 710.4758)
        if (!(fabs(Fspring) <= 1.7976931348623157e308)) Fspring = 0.0;
        fy = Fspring * (1 + dissipation * depthRate);
        const double mu_d = 1, latchvel = 0.05;
        const double mu = mu_d * tanh(vx / latchvel / 2);
        fx = -fy * mu;
        return;
    }
    const double depth = 0.0 - y;
    const double voidStiffness = 1.0;   // N/m
    const double vs = p[6];
    double transition;
    if (kind == MH_EXT_CONTACT_ACKERMANN_VAN_DEN_BOGERT) {
        fy = 0.0;
        if (depth > 0) fy = fmax(0.0, stiffness * (depth * depth * depth) * (1 + dissipation * depthRate));
        fy += voidStiffness * depth;
        transition = tanh(vx / vs / 2);
    } else {   // MH_EXT_CONTACT_ESPOSITO_MILLER
        const double d0sq = p[7] * p[7];
        const double dy = 0.5 * (sqrt(depth * depth + d0sq) + depth);
        fy = stiffness * (dy * dy) * (1 + dissipation * depthRate) + voidStiffness * depth;
        transition = tanh(vx / vs);
    }
    fx = -transition * p[5] * fy;
}

// The station's position P and velocity Vs in ground from its body's pose
// (R, o) and spatial velocity (w; v of the point at the ground origin): the
// expressions of the muscle path points.
__device__ __forceinline__ void contact_station(const double* R, const double* o, double w0, double w1, double w2,
        double v0, double v1, double v2, const double* __restrict__ loc, double* P, double* Vs) {
#pragma clang fp contract(off)
    const double l0 = loc[0], l1 = loc[1], l2 = loc[2];
    P[0] = o[0] + (R[0] * l0 + R[1] * l1 + R[2] * l2);
    P[1] = o[1] + (R[3] * l0 + R[4] * l1 + R[5] * l2);
    P[2] = o[2] + (R[6] * l0 + R[7] * l1 + R[8] * l2);
    Vs[0] = v0 + (w1 * P[2] - w2 * P[1]);
    Vs[1] = v1 + (w2 * P[0] - w0 * P[2]);
    Vs[2] = v2 + (w0 * P[1] - w1 * P[0]);
}

}  // namespace mh
