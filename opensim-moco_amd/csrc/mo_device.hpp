// mo_device.hpp -- the velocity-stage device functions the muscle-output
// kernels (muscle_outputs.hip) and the metabolics kernels (metabolics.hip)
// share (a lane's inputs where they lie are goal_lanes.hpp's PointIn): the
// forward kinematic pass over the bodies of a muscle's path, the path's length and lengthening speed, the
// muscle's own inputs and the directions that can change them.
#pragma once
#include "goal_lanes.hpp"

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
        const PointIn& in) {
    const int zo = M.presc ? 2 * M.nq : 0;
    const double exc = in[M.ns + M.mus_control[im]];
    const int sa = M.mus_act_state[im], sf = M.mus_ftn_state[im], id = M.mus_ider[im];
    const double act = sa >= 0 ? in[sa - zo] : exc;
    const double ftn = sf >= 0 ? in[sf - zo] : 0.0;
    const double dft = id >= 0 ? in[M.ns + M.nc + id] : 0.0;
    return dgf_output(M, im, which, L, S, act, exc, ftn, sf >= 0, id >= 0, dft);
}

// Every quantity of muscle im at once (dgf_outputs), its inputs picked as
// mo_value picks them: the bits of mo_value's outputs.
__device__ __forceinline__ DgfOut mo_all(const DevModel& M, int im, double L, double S, const PointIn& in) {
    const int zo = M.presc ? 2 * M.nq : 0;
    const double exc = in[M.ns + M.mus_control[im]];
    const int sa = M.mus_act_state[im], sf = M.mus_ftn_state[im], id = M.mus_ider[im];
    const double act = sa >= 0 ? in[sa - zo] : exc;
    const double ftn = sf >= 0 ? in[sf - zo] : 0.0;
    const double dft = id >= 0 ? in[M.ns + M.nc + id] : 0.0;
    return dgf_outputs(M, im, L, S, act, exc, ftn, sf >= 0, id >= 0, dft);
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
__device__ __forceinline__ void mo_with_kinematics(const DevModel& M, double t, const PointIn& in,
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
        const PointInAt u{in, M.nq};
        mo_kinematics<Z::MB>(M, in, u, mask, X, V);
        body(in, u);
    }
}
