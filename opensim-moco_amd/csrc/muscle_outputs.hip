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
#include "core.hpp"

// The point inputs of one grid point where they lie (x, or a probe row) with a
// lane's perturbation applied on the fly (lane_inputs' arithmetic: in[i] +
// step): states, controls and derivative variables, all the outputs read.
struct MoIn {
    const double* __restrict__ xs;
    const double* __restrict__ xc;
    const double* __restrict__ xd;
    int NS, NC, pi;
    double step;
    __device__ __forceinline__ double operator[](int i) const {
#pragma clang fp contract(off)
        const double v = i < NS ? xs[i] : (i < NS + NC ? xc[i - NS] : xd[i - NS - NC]);
        return i == pi ? v + step : v;
    }
};
struct MoInAt {
    const MoIn& in;
    int o;
    __device__ __forceinline__ double operator[](int j) const { return in[o + j]; }
};

// One body of the forward kinematic pass of dae_eval (dae_device.hpp),
// position and velocity parts: the parent's pose Pp and spatial velocity Vp (in
// ground about the ground origin) become body B's.  The position part is
// dae_eval's statement for statement; the velocity statements are its V
// updates (the terms of V only: no bias acceleration, no motion subspace).
template <class Q, class U>
__device__ __forceinline__ void mo_stage(const DevModel& M, const Q& q, const U& u, const mh_body& B,
        const Pose& Pp, const SV& Vp, Pose& Pb, SV& Vb) {
    double RGF[9], t0, t1, t2;
    mm3(Pp.R, B.R_PF, RGF);
    mv3(Pp.R, B.p_PF[0], B.p_PF[1], B.p_PF[2], t0, t1, t2);
    const double pGF0 = Pp.p[0] + t0, pGF1 = Pp.p[1] + t1, pGF2 = Pp.p[2] + t2;
    SV V = Vp;
    double pFM0 = 0, pFM1 = 0, pFM2 = 0;
    for (int a = B.axis_begin; a < B.axis_begin + B.axis_count; ++a) {
        const mh_axis X = M.axes[a];
        if (X.type != MH_AXIS_TRANSLATION) continue;
        double v, d1, d2;
        fn_eval(M, X.func, q, v, d1, d2);
        pFM0 += v * X.dir[0]; pFM1 += v * X.dir[1]; pFM2 += v * X.dir[2];
        const mh_function F = M.funcs[X.func];
        if (F.kind == MH_FN_CONSTANT) continue;
        double s0, s1, s2;
        mv3(RGF, X.dir[0], X.dir[1], X.dir[2], s0, s1, s2);
        const double thd = d1 * u[F.coord];
        V.v0 += s0 * thd; V.v1 += s1 * thd; V.v2 += s2 * thd;
    }
    mv3(RGF, pFM0, pFM1, pFM2, t0, t1, t2);
    const double oM0 = pGF0 + t0, oM1 = pGF1 + t1, oM2 = pGF2 + t2;
    double Rcur[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    for (int a = B.axis_begin; a < B.axis_begin + B.axis_count; ++a) {
        const mh_axis X = M.axes[a];
        if (X.type != MH_AXIS_ROTATION) continue;
        const mh_function F = M.funcs[X.func];
        double v, d1, d2;
        fn_eval(M, X.func, q, v, d1, d2);
        if (F.kind != MH_FN_CONSTANT) {
            double RGc[9], w0, w1, w2, s0, s1, s2;
            mm3(RGF, Rcur, RGc);
            mv3(RGc, X.dir[0], X.dir[1], X.dir[2], w0, w1, w2);
            cross3(oM0, oM1, oM2, w0, w1, w2, s0, s1, s2);
            const double thd = d1 * u[F.coord];
            V.w0 += w0 * thd; V.w1 += w1 * thd; V.w2 += w2 * thd;
            V.v0 += s0 * thd; V.v1 += s1 * thd; V.v2 += s2 * thd;
        }
        double Rk[9];
        axis_rot(X.dir[0], X.dir[1], X.dir[2], v, Rk);
        mm3(Rcur, Rk, Rcur);
    }
    double RGM[9];
    mm3(RGF, Rcur, RGM);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Pb.R[3 * i + j] = RGM[3 * i] * B.R_BM[3 * j] + RGM[3 * i + 1] * B.R_BM[3 * j + 1] +
                              RGM[3 * i + 2] * B.R_BM[3 * j + 2];
    mv3(Pb.R, B.p_BM[0], B.p_BM[1], B.p_BM[2], t0, t1, t2);
    Pb.p[0] = oM0 - t0; Pb.p[1] = oM1 - t1; Pb.p[2] = oM2 - t2;
    Vb = V;
}

// The bodies whose pose muscle im's path reads (bit b = body b): those of its
// path points and wrap surfaces with all their ancestors.  MB <= 32 in every
// size class, so a 64-bit mask holds them (mo_kinematics asserts it for every
// kernel that uses the mask).
__device__ __forceinline__ unsigned long long mo_muscle_bodies(const DevModel& M, int im) {
    unsigned long long mask = 0ull;
    const mh_muscle& mu = M.mus[im];
    for (int i = mu.point_begin; i < mu.point_begin + mu.point_count; ++i)
        for (int b = M.pts[i].body, n = 0; b >= 0 && n <= M.nb; b = M.bodies[b].parent, ++n) mask |= 1ull << b;
    if (M.mus_pw_count)
        for (int k = M.mus_pw_begin[im]; k < M.mus_pw_begin[im] + M.mus_pw_count[im]; ++k)
            for (int b = M.wr[M.pw[k].wrap].body, n = 0; b >= 0 && n <= M.nb; b = M.bodies[b].parent, ++n)
                mask |= 1ull << b;
    return mask;
}

// The kinematic pass restricted to the bodies of `mask` (closed under
// parents; the bodies are in topological order, as dae_eval assumes): X[b + 1]
// and V[b + 1] of those bodies, X[0] / V[0] the ground's.
template <int MB, class Q, class U>
__device__ __forceinline__ void mo_kinematics(const DevModel& M, const Q& q, const U& u, unsigned long long mask,
        Pose* X, SV* V) {
    static_assert(MB < 64, "mo_muscle_bodies holds the bodies in a 64-bit mask");
    X[0] = Pose{{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}};
    V[0] = sv_zero();
    for (int b = 0; b < M.nb && b < MB; ++b) {
        if (!((mask >> b) & 1ull)) continue;
        const mh_body& B = M.bodies[b];
        mo_stage(M, q, u, B, X[B.parent + 1], V[B.parent + 1], X[b + 1], V[b + 1]);
    }
}

// Muscle im's current path, its length L and lengthening speed S: dae_eval's
// muscle loop up to the call of dgf_eval (conditional and moving points, the
// point velocities, dev_apply_wraps, the length / speed sums).
template <int MP, class Q, class U>
__device__ __forceinline__ void mo_path(const DevModel& M, int im, const Q& q, const U& u, const Pose* X,
        const SV* V, double& L, double& S) {
    const mh_muscle& mu = M.mus[im];
    CPath<MP> C;
    int np = 0;
    for (int i = mu.point_begin; i < mu.point_begin + mu.point_count && np < MP; ++i) {
        const mh_path_point pt = M.pts[i];
        double l0 = pt.loc[0], l1 = pt.loc[1], l2 = pt.loc[2];
        double dl0 = 0, dl1 = 0, dl2 = 0;
        if (pt.kind == MH_PP_CONDITIONAL) {
            const double qv = q[pt.coord];
            if (!(qv >= pt.range[0] && qv <= pt.range[1])) continue;
        } else if (pt.kind == MH_PP_MOVING) {
            double v, d1, d2;
            if (pt.fx >= 0) {
                fn_eval(M, pt.fx, q, v, d1, d2); l0 = v;
                const mh_function F = M.funcs[pt.fx];
                if (F.kind != MH_FN_CONSTANT) dl0 = d1 * u[F.coord];
            }
            if (pt.fy >= 0) {
                fn_eval(M, pt.fy, q, v, d1, d2); l1 = v;
                const mh_function F = M.funcs[pt.fy];
                if (F.kind != MH_FN_CONSTANT) dl1 = d1 * u[F.coord];
            }
            if (pt.fz >= 0) {
                fn_eval(M, pt.fz, q, v, d1, d2); l2 = v;
                const mh_function F = M.funcs[pt.fz];
                if (F.kind != MH_FN_CONSTANT) dl2 = d1 * u[F.coord];
            }
        }
        const int bs = pt.body + 1;
        const Pose& Pb = X[bs];
        double t0, t1, t2, r0, r1, r2;
        mv3(Pb.R, l0, l1, l2, t0, t1, t2);
        C.P[np][0] = Pb.p[0] + t0; C.P[np][1] = Pb.p[1] + t1; C.P[np][2] = Pb.p[2] + t2;
        const SV& Vb = V[bs];
        cross3(Vb.w0, Vb.w1, Vb.w2, C.P[np][0], C.P[np][1], C.P[np][2], t0, t1, t2);
        mv3(Pb.R, dl0, dl1, dl2, r0, r1, r2);
        C.V[np][0] = Vb.v0 + t0 + r0; C.V[np][1] = Vb.v1 + t1 + r1; C.V[np][2] = Vb.v2 + t2 + r2;
        C.pt[np] = i;
        C.pwi[np] = -1;
        C.body[np] = pt.body;
        C.wlen[np] = 0.0;
        ++np;
    }
    C.n = np;
    if (M.mus_pw_count && M.mus_pw_count[im] > 0) {
        auto active = [&](int i) {
            for (int k = 0; k < C.n; ++k)
                if (C.pt[k] == i) return true;
            return false;
        };
        dev_apply_wraps<MP>(M, im, X, V, active, C);
        np = C.n;
    }
    L = 0.0;
    S = 0.0;
    for (int k = 1; k < np; ++k) {
        const double d0 = C.P[k][0] - C.P[k - 1][0], d1 = C.P[k][1] - C.P[k - 1][1], d2 = C.P[k][2] - C.P[k - 1][2];
        const double l = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
        if (C.arc(k)) L += C.wlen[k];
        else L += l;
        const double e0 = C.V[k][0] - C.V[k - 1][0], e1 = C.V[k][1] - C.V[k - 1][1],
                     e2 = C.V[k][2] - C.V[k - 1][2];
        S += (d0 * e0 + d1 * e1 + d2 * e2) / l;
    }
}

// Output `which` of muscle im from its length and speed and the lane's inputs:
// the muscle's inputs picked as dae_eval picks them (mus_act_state and
// mus_ftn_state index [q, u, z]; with prescribed kinematics the NLP states are
// z alone).
__device__ __forceinline__ double mo_value(const DevModel& M, int im, int which, double L, double S,
        const MoIn& in) {
    const int zo = M.presc ? 2 * M.nq : 0;
    const double exc = in[M.ns + M.mus_control[im]];
    const int sa = M.mus_act_state[im], sf = M.mus_ftn_state[im], id = M.mus_ider[im];
    const double act = sa >= 0 ? in[sa - zo] : exc;
    const double ftn = sf >= 0 ? in[sf - zo] : 0.0;
    const double dft = id >= 0 ? in[M.ns + M.nc + id] : 0.0;
    return dgf_output(M, im, which, L, S, act, exc, ftn, sf >= 0, id >= 0, dft);
}

// Whether direction dir (0 = t0, 1 = tf, 2 + i = point input i) can change
// output `which` of muscle im: the times, the coordinate values and speeds
// (states 0 .. 2 nq; none with prescribed kinematics), the muscle's activation
// state -- its excitation control when it has none, or when the output is the
// excitation itself --, its normalized-tendon-force state and its tendon-force
// derivative variable.
__device__ __forceinline__ bool mo_live(const DevModel& M, int im, int which, int dir) {
    if (dir < 2) return true;
    const int i = dir - 2;
    const int zo = M.presc ? 2 * M.nq : 0;
    if (!M.presc && i < 2 * M.nq) return true;
    const int sa = M.mus_act_state[im], sf = M.mus_ftn_state[im], id = M.mus_ider[im];
    if (sa >= 0 && i == sa - zo) return true;
    if ((sa < 0 || which == MH_MO_EXCITATION) && i == M.ns + M.mus_control[im]) return true;
    if (sf >= 0 && i == sf - zo) return true;
    if (id >= 0 && i == M.ns + M.nc + id) return true;
    return false;
}

// The kinematics of one lane: q and u where they lie (the iterate or a probe
// row, perturbed on the fly), or with prescribed kinematics the kinematics
// table's at the lane's time, as GenericDae::eval_w takes them.
template <class Z, class F>
__device__ __forceinline__ void mo_with_kinematics(const DevModel& M, double t, const MoIn& in,
        unsigned long long mask, Pose* X, SV* V, const F& body) {
    if (M.presc) {
        double q[Z::MQ], u[Z::MQ];
        for (int j = 0; j < Z::MQ; ++j) {
            q[j] = 0.0; u[j] = 0.0;
            if (j < M.nq) {
                double ud;
                table_eval_d(M, M.kin_table, M.kin_col[j], t, q[j], u[j], ud);
            }
        }
        mo_kinematics<Z::MB>(M, q, u, mask, X, V);
        body(q, u);
    } else {
        const MoInAt u{in, M.nq};
        mo_kinematics<Z::MB>(M, in, u, mask, X, V);
        body(in, u);
    }
}

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
