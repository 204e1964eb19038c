// contact.hip -- mh_eval_contact_forces: the station-plane contact forces of
// a model (mh_external_force records of kind 1..3) along a solution.  A
// velocity-stage kernel on muscle_outputs.hip's kinematic pass (mo_device.hpp)
// restricted to the bodies that carry a station, and the force function
// dae_eval calls (contact_device.hpp).  No dynamics run.  One instantiation
// per size class.  A translation unit of its own, as metabolics.hip.
#include "mo_device.hpp"

// The bodies whose pose the model's contact stations read, with all their
// ancestors (bit b = body b).
__device__ __forceinline__ unsigned long long contact_bodies(const DevModel& M) {
    unsigned long long mask = 0ull;
    for (int e = 0; e < M.next; ++e) {
        if (M.ext[e].kind == MH_EXT_TABLE) continue;
        for (int b = M.ext[e].body, n = 0; b >= 0 && n <= M.nb; b = M.bodies[b].parent, ++n) mask |= 1ull << b;
    }
    return mask;
}

// One thread per input row [time, NI point inputs]: for each contact record,
// in record order, the force on the body at the station in ground, the
// station's position and its velocity in ground (9 values).
template <class Z>
__global__ void __launch_bounds__(64) k_contact_forces(DevModel M, Layout L, int ncontacts, int npts,
        const double* __restrict__ inp, double* __restrict__ outp) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npts) return;
    const double* row = inp + (long)p * (1 + L.NI);
    const PointIn in{row + 1, row + 1 + L.NS, row + 1 + L.NS + L.NC, L.NS, L.NC, -1, 0.0};
    Pose X[Z::MB + 1];
    SV V[Z::MB + 1];
    double* out = outp + (long)p * ncontacts * 9;
    mo_with_kinematics<Z>(M, row[0], in, contact_bodies(M), X, V, [&](const auto&, const auto&) {
        int k = 0;
        for (int e = 0; e < M.next && k < ncontacts; ++e) {
            const mh_external_force E = M.ext[e];
            if (E.kind == MH_EXT_TABLE) continue;
            const int bs = E.body + 1;
            if (bs < 1 || bs > Z::MB) continue;
            const double* cp = M.coef + E.force_col;
            const SV& Vb = V[bs];
            double P[3], Vs[3], fx, fy;
            contact_station(X[bs].R, X[bs].p, Vb.w0, Vb.w1, Vb.w2, Vb.v0, Vb.v1, Vb.v2, cp, P, Vs);
            contact_force(E.kind, cp, P[1], Vs[1], Vs[0], fx, fy);
            double* o = out + 9 * k++;
            o[0] = fx; o[1] = fy; o[2] = 0.0;
            for (int i = 0; i < 3; ++i) { o[3 + i] = P[i]; o[6 + i] = Vs[i]; }
        }
    });
}

template <class Z>
static void be_contact_forces(mh_ctx* c, int np, const double* in, double* out) {
    Layout L = make_layout(c, 0, 0);
    hipLaunchKernelGGL(k_contact_forces<Z>, dim3((np + 63) / 64), dim3(64), 0, c->stream, c->M, L, c->ncontacts, np,
            in, out);
}

void contact_forces_probe(mh_ctx* c, int np, const double* in, double* out) {
    static constexpr decltype(&be_contact_forces<SzSmall>) kProbe[4] = {
        &be_contact_forces<SzSmall>, &be_contact_forces<SzMedium>, &be_contact_forces<SzLarge>,
        &be_contact_forces<SzBody>};
    kProbe[c->size_class](c, np, in, out);
}
