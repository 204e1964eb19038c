// muscle_outputs.hip -- MocoOutputGoal over a DeGrooteFregly2016Muscle output
// (include/mocohip.h MH_GOAL_OUTPUT, enum mh_muscle_output) and
// mh_eval_muscle_outputs: a velocity-stage kernel.  Per thread (one goal at one
// lane) the poses and spatial velocities of the bodies its muscle's path
// touches, the path with its length and lengthening speed, and dgf_output
// (dae_device.hpp).  No
// Newton-Euler backward pass, no mass matrix, no dae_eval: the kernel works
// with prescribed kinematics and costs a fraction of a dynamics lane.  One
// instantiation per size class, selected by muscle_outputs_backends()
// [size_class] whatever back end serves g and J.  A translation unit of its
// own, as joint_reaction.hip: generic.hip compiles to the code it had
// without it.
#include "mo_device.hpp"

// One thread per (goal of kind 17, grid point, lane), the goal slowest so that
// a wave works on one muscle, the lanes in the Lanes layout of k_eval (ND = NI
// - NSL + 2: the slack inputs get no lane): L = value / divisor of goal j of nmo
// (in goal order) to lv[(k stride + lane) nmo + j] where the lane's direction
// is live for the goal (mo_live; the base lane always); any other thread
// returns at once.  C (objective mode, base lanes only: stride 1):
// C[k ngoals + g] = quad[k] L.  The kinematic pass covers the bodies of the
// goal's muscle only; poses and velocities are indexed by body
// (dev_apply_wraps reads them so), in scratch for the larger size classes.
template <class Z>
__global__ void __launch_bounds__(64) k_muscle_outputs(DevModel M, Layout L, Lanes Ln, GoalSet GS, int nmo,
        const double* __restrict__ x, const double* __restrict__ grid, const double* __restrict__ quad,
        double* __restrict__ C, double* __restrict__ lv) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nlanes = (long)L.G * Ln.stride;
    if (gid >= nlanes * nmo) return;
    const int j = (int)(gid / nlanes);
    const long lane = gid - (long)j * nlanes;
    const int k = (int)(lane / Ln.stride);
    const int r = (int)(lane - (long)k * Ln.stride);
    const bool base = r == Ln.base;
    const int dir = r >= Ln.ND ? r - Ln.ND : r;
    int g = -1;
    for (int i = 0, n = 0; i < GS.ngoals && g < 0; ++i)
        if (GS.goals[i].kind == MH_GOAL_OUTPUT && n++ == j) g = i;
    if (g < 0) return;
    const int tb = GS.goals[g].term_begin, im = GS.gidx[tb], which = GS.gcol[tb];
    if (!base && !mo_live(M, im, which, dir)) return;
    MoIn in{x + 2 + (long)k * L.NS, x + 2 + (long)L.NS * L.G + (long)k * L.NC, x + L.DB + (long)k * L.NDV, L.NS, L.NC,
            -1, 0.0};
    const double t = lane_time(Ln, grid[k], x[0], x[1], r, in.pi, in.step);
    Pose X[Z::MB + 1];
    SV V[Z::MB + 1];
    mo_with_kinematics<Z>(M, t, in, mo_muscle_bodies(M, im), X, V, [&](const auto& q, const auto& u) {
#pragma clang fp contract(off)
        double Lm, Sm;
        mo_path<Z::MP>(M, im, q, u, X, V, Lm, Sm);
        const double Lg = mo_value(M, im, which, Lm, Sm, in) / GS.gw[tb];
        lv[lane * nmo + j] = Lg;
        if (C) C[(long)k * GS.ngoals + g] = quad[k] * Lg;
    });
}

// One thread per (grid point, direction): the quotients of k_muscle_outputs'
// lane values with k_grad's formulas and arithmetic, G.weight * dur * quad[k]
// * dL of the goals the direction is live for, added to what the other goal
// kernels left in grad / tpart (after them on the same stream: one writer per
// entry and launch); direction 0 also writes the goals' integrand slots of C.
// A direction live for no goal writes nothing: its entry keeps its bits.
__global__ void __launch_bounds__(64) k_muscle_outputs_grad(DevModel M, Layout L, Lanes Ln, GoalSet GS, int nmo,
        const double* __restrict__ x, const double* __restrict__ quad, const double* __restrict__ lv,
        double* __restrict__ C, double* __restrict__ grad, double* __restrict__ tpart) {
#pragma clang fp contract(off)
    const int ND = Ln.ND;
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= (long)L.G * ND) return;
    const int k = (int)(tid / ND), d = (int)(tid % ND);
    const double dur = x[1] - x[0], h = Ln.h;
    const double* lk = lv + (long)k * Ln.stride * nmo;
    double acc = 0.0;
    bool any = false;
    int j = 0;
    for (int g = 0; g < GS.ngoals && j < nmo; ++g) {
        const mh_goal G = GS.goals[g];
        if (G.kind != MH_GOAL_OUTPUT) continue;
        const int tb = G.term_begin;
        if (mo_live(M, GS.gidx[tb], GS.gcol[tb], d)) {
            const double l0 = lk[(long)Ln.base * nmo + j], l1 = lk[(long)d * nmo + j];
            const double dL = Ln.fd == MH_FD_CENTRAL ? (l1 - lk[(long)(ND + d) * nmo + j]) / (2.0 * h)
                            : (Ln.fd == MH_FD_FORWARD ? (l1 - l0) / h : (l0 - l1) / h);
            acc += G.weight * dur * quad[k] * dL;
            any = true;
            if (d == 0) C[(long)k * GS.ngoals + g] = quad[k] * l0;
        }
        ++j;
    }
    if (!any) return;
    if (d < 2) tpart[(long)k * 2 + d] += acc;
    else if (d - 2 < L.NS) grad[2 + (long)k * L.NS + (d - 2)] += acc;
    else if (d - 2 < L.NS + L.NC) grad[2 + (long)L.NS * L.G + (long)k * L.NC + (d - 2 - L.NS)] += acc;
    else if (d - 2 < L.NS + L.NC + L.NDV) grad[L.DB + (long)k * L.NDV + (d - 2 - L.NS - L.NC)] += acc;
    else grad[L.XM + (long)k * L.NM + (d - 2 - L.NS - L.NC - L.NDV)] += acc;
}

// mh_eval_muscle_outputs: one thread per input row [time, NI point inputs],
// output which[o] of muscle mus[o] to outp[row nout + o]; one kinematic pass
// per row over the bodies of all the requested muscles.
template <class Z>
__global__ void __launch_bounds__(64) k_muscle_outputs_probe(DevModel M, Layout L, int nout,
        const int* __restrict__ mus, const int* __restrict__ which, int npts, const double* __restrict__ inp,
        double* __restrict__ outp) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npts) return;
    const double* row = inp + (long)p * (1 + L.NI);
    const MoIn in{row + 1, row + 1 + L.NS, row + 1 + L.NS + L.NC, L.NS, L.NC, -1, 0.0};
    unsigned long long mask = 0ull;
    for (int o = 0; o < nout; ++o) mask |= mo_muscle_bodies(M, mus[o]);
    Pose X[Z::MB + 1];
    SV V[Z::MB + 1];
    mo_with_kinematics<Z>(M, row[0], in, mask, X, V, [&](const auto& q, const auto& u) {
        int last = -1;
        double Lm = 0.0, Sm = 0.0;
        for (int o = 0; o < nout; ++o) {
            if (mus[o] != last) {   // (consecutive outputs of one muscle share its path)
                last = mus[o];
                mo_path<Z::MP>(M, last, q, u, X, V, Lm, Sm);
            }
            outp[(long)p * nout + o] = mo_value(M, last, which[o], Lm, Sm, in);
        }
    });
}

template <class Z>
static void be_muscle_outputs(mh_ctx* c, const double* x, int mode) {
    Layout L = make_layout(c, 0, c->G);
    if (mode == 0) {
        // base lanes only
        const Lanes ln{c->fd, c->lanes_mo.ND, 1, 0, c->h};
        hipLaunchKernelGGL(k_muscle_outputs<Z>, dim3((unsigned)(((long)c->G * c->nmo + 63) / 64)), dim3(64), 0,
                c->stream, c->M, L, ln, c->GS, c->nmo, x, c->d_grid, c->d_quad, c->d_C, c->d_mo);
        return;
    }
    const Lanes& ln = c->lanes_mo;
    const long lanes = (long)c->G * ln.stride, dirs = (long)c->G * ln.ND;
    hipLaunchKernelGGL(k_muscle_outputs<Z>, dim3((unsigned)((lanes * c->nmo + 63) / 64)), dim3(64), 0, c->stream, c->M,
            L, ln, c->GS, c->nmo, x, c->d_grid, c->d_quad, (double*)nullptr, c->d_mo);
    hipLaunchKernelGGL(k_muscle_outputs_grad, dim3((unsigned)((dirs + 63) / 64)), dim3(64), 0, c->stream, c->M, L,
            ln, c->GS, c->nmo, x, c->d_quad, c->d_mo, c->d_C, c->d_grad, c->d_tpart);
}
template <class Z>
static void be_muscle_outputs_probe(mh_ctx* c, int nout, const int* mus, const int* which, int np,
        const double* in, double* out) {
    Layout L = make_layout(c, 0, 0);
    hipLaunchKernelGGL(k_muscle_outputs_probe<Z>, dim3((np + 63) / 64), dim3(64), 0, c->stream, c->M, L, nout, mus,
            which, np, in, out);
}

const MuscleOutputsBackend* muscle_outputs_backends() {
    static const MuscleOutputsBackend kMuscleOutputs[4] = {
        {&be_muscle_outputs<SzSmall>, &be_muscle_outputs_probe<SzSmall>},
        {&be_muscle_outputs<SzMedium>, &be_muscle_outputs_probe<SzMedium>},
        {&be_muscle_outputs<SzLarge>, &be_muscle_outputs_probe<SzLarge>},
        {&be_muscle_outputs<SzBody>, &be_muscle_outputs_probe<SzBody>},
    };
    return kMuscleOutputs;
}
