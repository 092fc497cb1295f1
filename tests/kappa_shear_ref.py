"""Calculate_kappa_shear (src/parameterizations/vertical/MOM_kappa_shear.F90:133-411) with kappa_shear_column (:864-1372),
calculate_projected_state (:1377-1504) and find_kappa_tke (:1507-2067), Boussinesq, and find_uv_at_h without vertical mixing
(MOM_diabatic_aux.F90:546-571, :595-611), restated per column in plain Python from the Fortran in its statement order.  The
arithmetic is + - * / and sqrt; x**2 is a product; MAX and MIN return their first argument on a tie (fmax1, fmin1), except at the
one kind of site where the tie shows, N2 = MAX(0.0, ...) of :1492-1502 with an argument of -0.0, where the compiled reference
returns its second (dmax: N2 = -0.0; found by tests/test_ref_parity_cpu.py with the case `tie`).  The column's arrays are lists
indexed as in the Fortran (element 0 is not used) and start as NaN, so that a read of a value the reference never set shows.

The constants tke_noflux_top_BC, tke_noflux_bottom_BC and debug_soln of find_kappa_tke are .false. in the reference; their arms
are not restated.  Density derivatives come from the oracle's EOS (tests/ref_common._derivs), which is held to the compiled Fortran.

BRANCHES names the arms a case list can be held to; every run adds to a dict of counters.

What pins this file: tests/test_ref_parity_cpu.py compares it, whole arrays bit for bit, with the reference's own
MOM_kappa_shear.F90 and MOM_EOS.F90 compiled where they lie (oracle/Makefile), on every case of CASES, through the reference's own
kappa_shear_init, EOS_init and unit_scaling_init, and with the results recorded from them (tests/golden/ref_kshear_*.npz).  Outside
that comparison stay find_uv_at_h below (its module is not compiled; the compiled routine is handed what it makes) and the
iteration count KS_its (it reaches no diagnostic of the reference); tests/test_kappa_shear_cpu.py holds those."""
import math

import numpy as np

from mom6_amd import abi
from tests.ref_common import _derivs

G = abi.G
NAN = float("nan")

BRANCHES = ("land", "uv_plain", "uv_zero_mix", "layered", "eos", "elim_on", "elim_off", "merged", "kf_pos", "nzc_1", "nkml_gt1",
            "no_mixing_exit", "pred_corr", "last_iteration", "halved", "halving_ran_out", "refine_accept", "refine_reject",
            "two_iterations", "tol_restrictive", "tol_loose", "scan_stable_arm", "scan_stable_invalid", "no_source", "newton_entered",
            "newton_aborted", "newton_pivot_K", "newton_pivot_Q", "newton_left_early", "newton_K_Q", "dKdQ_bug", "dKdQ_fixed",
            "all_layer_bug", "all_layer_avg", "ke_tke_interior", "kappa_trunc_bottom", "kappa_trunc_top", "kappa_small_fwd",
            "kappa_small_bwd", "vel_underflow", "itt_limit", "lz_rescale")
DIAG_3D = ("N2_init", "S2_init", "N2_mean", "S2_mean")
DIAG_2D = ("KS_its",)


def fmax1(a, b):
    return b if b > a else a


def fmin1(a, b):
    return b if b < a else a


def dmax(a, b):
    """MAX(a, b) as the compiled reference evaluates it: the second argument on a tie, which between +0 and -0 is the sign."""
    return a if a > b else b


def new_counts():
    return dict.fromkeys(BRANCHES, 0)


def find_uv_at_h(d, M, GV, u, v, h, zero_mix, br=None):
    """find_uv_at_h without ea and eb: the plain average (:607-610) or, with zero_mix, the arm of :595-605.  Returns u_h, v_h of
    nk levels, set on the computational domain."""
    nz = d.nk
    aCu = M[G["areaCu"]]; aCv = M[G["areaCv"]]; IaT = M[G["IareaT"]]
    u_h = np.full(h.shape, np.nan); v_h = np.full(h.shape, np.nan)
    h_neglect = GV.H_subroundoff
    for jl in range(d.nj):
        for il in range(d.ni):
            j = jl + d.joff; i = il + d.ioff
            a_w = a_e = a_s = a_n = 0.0
            sum_area = float(aCu[j, i - 1]) + float(aCu[j, i])
            if sum_area > 0.0:
                Idenom = math.sqrt(0.5 * float(IaT[j, i]) / sum_area)
                a_w = float(aCu[j, i - 1]) * Idenom; a_e = float(aCu[j, i]) * Idenom
            sum_area = float(aCv[j - 1, i]) + float(aCv[j, i])
            if sum_area > 0.0:
                Idenom = math.sqrt(0.5 * float(IaT[j, i]) / sum_area)
                a_s = float(aCv[j - 1, i]) * Idenom; a_n = float(aCv[j, i]) * Idenom
            for k in range(nz):
                ue, uw = float(u[k, j, i]), float(u[k, j, i - 1])
                vn, vs = float(v[k, j, i]), float(v[k, j - 1, i])
                if zero_mix:
                    hk = float(h[k, j, i])
                    b1 = 1.0 / (hk + h_neglect)
                    if k == 0:
                        u_h[k, j, i] = (hk * b1) * ((a_e * ue) + (a_w * uw))
                        v_h[k, j, i] = (hk * b1) * ((a_n * vn) + (a_s * vs))
                    else:
                        u_h[k, j, i] = (hk * ((a_e * ue) + (a_w * uw))) * b1
                        v_h[k, j, i] = (hk * ((a_n * vn) + (a_s * vs))) * b1
                else:
                    u_h[k, j, i] = (a_e * ue) + (a_w * uw)
                    v_h[k, j, i] = (a_n * vn) + (a_s * vs)
            if br is not None:
                br["uv_zero_mix" if zero_mix else "uv_plain"] += 1
    return u_h, v_h


def calculate_projected_state(kappa, u0, v0, T0, S0, dt, nz, dz, I_dz_int, dbuoy_dT, dbuoy_dS, vel_under, u, v, T, Sal, N2, S2,
                              L_to_Z, br, ks_int=None, ke_int=None):
    """:1377-1504"""
    ks = 1; ke = nz
    if ks_int is not None:
        ks = max(ks_int - 1, 1)
    if ke_int is not None:
        ke = min(ke_int, nz)
    if ks > ke:
        return
    c1 = [NAN] * (nz + 2)
    if dt > 0.0:
        a_b = dt * (kappa[ks + 1] * I_dz_int[ks + 1])
        b1 = 1.0 / (dz[ks] + a_b)
        c1[ks + 1] = a_b * b1; d1 = dz[ks] * b1
        u[ks] = (b1 * dz[ks]) * u0[ks]; v[ks] = (b1 * dz[ks]) * v0[ks]
        T[ks] = (b1 * dz[ks]) * T0[ks]; Sal[ks] = (b1 * dz[ks]) * S0[ks]
        for k in range(ks + 1, ke):
            a_a = a_b
            a_b = dt * (kappa[k + 1] * I_dz_int[k + 1])
            bd1 = dz[k] + d1 * a_a
            b1 = 1.0 / (bd1 + a_b)
            c1[k + 1] = a_b * b1; d1 = bd1 * b1
            u[k] = b1 * (dz[k] * u0[k] + a_a * u[k - 1])
            v[k] = b1 * (dz[k] * v0[k] + a_a * v[k - 1])
            T[k] = b1 * (dz[k] * T0[k] + a_a * T[k - 1])
            Sal[k] = b1 * (dz[k] * S0[k] + a_a * Sal[k - 1])
        a_a = a_b
        b1 = 1.0 / (dz[ke] + d1 * a_a)
        T[ke] = b1 * (dz[ke] * T0[ke] + a_a * T[ke - 1])
        Sal[ke] = b1 * (dz[ke] * S0[ke] + a_a * Sal[ke - 1])
        if ke == nz:
            a_b = dt * (kappa[nz + 1] * I_dz_int[nz + 1])
            b1nz_0 = 1.0 / ((dz[nz] + d1 * a_a) + a_b)
        else:
            b1nz_0 = b1
        u[ke] = b1nz_0 * (dz[ke] * u0[ke] + a_a * u[ke - 1])
        v[ke] = b1nz_0 * (dz[ke] * v0[ke] + a_a * v[ke - 1])
        if abs(u[ke]) < vel_under:
            u[ke] = 0.0; br["vel_underflow"] += 1
        if abs(v[ke]) < vel_under:
            v[ke] = 0.0; br["vel_underflow"] += 1
        for k in range(ke - 1, ks - 1, -1):
            u[k] = u[k] + c1[k + 1] * u[k + 1]
            v[k] = v[k] + c1[k + 1] * v[k + 1]
            if abs(u[k]) < vel_under:
                u[k] = 0.0; br["vel_underflow"] += 1
            if abs(v[k]) < vel_under:
                v[k] = 0.0; br["vel_underflow"] += 1
            T[k] = T[k] + c1[k + 1] * T[k + 1]
            Sal[k] = Sal[k] + c1[k + 1] * Sal[k + 1]
    else:
        for k in range(1, nz + 1):
            u[k] = u0[k]; v[k] = v0[k]; T[k] = T0[k]; Sal[k] = S0[k]
            if abs(u[k]) < vel_under:
                u[k] = 0.0; br["vel_underflow"] += 1
            if abs(v[k]) < vel_under:
                v[k] = 0.0; br["vel_underflow"] += 1

    def sq(x):
        return x * x
    S2[1] = 0.0; S2[nz + 1] = 0.0
    if ks > 1:
        S2[ks] = (sq(u[ks] - u0[ks - 1]) + sq(v[ks] - v0[ks - 1])) * sq(L_to_Z * I_dz_int[ks])
    for K in range(ks + 1, ke + 1):
        S2[K] = (sq(u[K] - u[K - 1]) + sq(v[K] - v[K - 1])) * sq(L_to_Z * I_dz_int[K])
    if ke < nz:
        S2[ke + 1] = (sq(u0[ke + 1] - u[ke]) + sq(v0[ke + 1] - v[ke])) * sq(L_to_Z * I_dz_int[ke + 1])
    N2[1] = 0.0; N2[nz + 1] = 0.0
    if ks > 1:
        N2[ks] = dmax(0.0, I_dz_int[ks] * (dbuoy_dT[ks] * (T0[ks - 1] - T[ks]) + dbuoy_dS[ks] * (S0[ks - 1] - Sal[ks])))
    for K in range(ks + 1, ke + 1):
        N2[K] = dmax(0.0, I_dz_int[K] * (dbuoy_dT[K] * (T[K - 1] - T[K]) + dbuoy_dS[K] * (Sal[K - 1] - Sal[K])))
    if ke < nz:
        N2[ke + 1] = dmax(0.0, I_dz_int[ke + 1] * (dbuoy_dT[ke + 1] * (T[ke] - T0[ke + 1]) + dbuoy_dS[ke + 1] * (Sal[ke] - S0[ke + 1])))


def find_kappa_tke(CS, N2, S2, kappa_in, Idz, h_Int, dz_Int, dz_h_Int, I_L2_bdry, f2, nz, K_Q, tke, kappa, br, kappa_src=None,
                   local_src=None):
    """:1507-2067.  dz_h_Int is the Boussinesq constant GV%H_to_Z.  Returns the iterations made (0: no source anywhere)."""
    n2 = nz + 2
    aQ = [NAN] * n2; dQdz = [NAN] * n2; dK = [NAN] * n2; dQ = [NAN] * n2; cQ = [NAN] * n2; cK = [NAN] * n2; I_Ld2 = [NAN] * n2
    TKE_decay = [NAN] * n2; k_src = [NAN] * n2; dQmdK = [NAN] * n2; dKdQ = [NAN] * n2; e1 = [NAN] * n2
    roundoff = 1.0e-16
    c_N2 = CS.C_N * CS.C_N; c_S2 = CS.C_S * CS.C_S
    q0 = CS.TKE_bg; kappa0 = CS.kappa_0
    TKE_min = fmax1(CS.TKE_bg, 1.0E-20 * (CS.m_to_Z * CS.m_to_Z) * (CS.T_to_s * CS.T_to_s))
    Ri_crit = CS.RiNo_crit
    Ilambda2 = 1.0 / (CS.lambda_ * CS.lambda_)
    kappa_trunc = CS.kappa_trunc
    do_Newton = False; abort_Newton = False
    tol_err = CS.kappa_tol_err
    Newton_err = 0.2
    ks_kappa = 2; ke_kappa = nz; ks_kappa_prev = 2; ke_kappa_prev = nz
    ke_src = 0; ks_src = nz + 1
    for K in range(2, nz + 1):
        if N2[K] < Ri_crit * S2[K]:
            k_src[K] = (2.0 * CS.Shearmix_rate * math.sqrt(S2[K])) * \
                ((Ri_crit * S2[K] - N2[K]) / (Ri_crit * S2[K] + CS.FRi_curvature * N2[K]))
            ke_src = K
            if ks_src > K:
                ks_src = K
        else:
            k_src[K] = 0.0
    if ks_src > ke_src:
        br["no_source"] += 1
        for K in range(1, nz + 2):
            kappa[K] = 0.0; K_Q[K] = 0.0; tke[K] = TKE_min
        if kappa_src is not None:
            for K in range(1, nz + 2):
                kappa_src[K] = 0.0
        if local_src is not None:
            for K in range(1, nz + 2):
                local_src[K] = 0.0
        return 0
    for K in range(1, nz + 2):
        kappa[K] = kappa_in[K]
        TKE_decay[K] = math.sqrt(c_N2 * N2[K] + c_S2 * S2[K])
        if (kappa[K] > 0.0) and (K_Q[K] > 0.0):
            tke[K] = kappa[K] / K_Q[K]
        else:
            tke[K] = TKE_min
    kappa[1] = 0.0; kappa[nz + 1] = 0.0
    eden2 = kappa0 * Idz[nz]
    e1[nz + 1] = 0.0; ome = 1.0
    for k in range(nz, 1, -1):
        eden1 = h_Int[k] * TKE_decay[k] + ome * eden2
        eden2 = kappa0 * Idz[k - 1]
        I_eden = 1.0 / (eden2 + eden1)
        e1[k] = eden2 * I_eden; ome = eden1 * I_eden
    e1[1] = 0.0

    its = 0
    for itt in range(1, CS.max_RiNo_it + 1):
        its = itt
        if not do_Newton:
            ke_tke = max(ke_kappa, ke_kappa_prev) + 1
            for k in range(1, min(ke_tke, nz) + 1):
                aQ[k] = (0.5 * (kappa[k] + kappa[k + 1]) + kappa0) * Idz[k]
            dQ[1] = -tke[1]
            tke[1] = q0; cQ[2] = 0.0; cQcomp = 1.0
            for K in range(2, ke_tke):
                dQ[K] = -tke[K]
                tke_src = dz_h_Int * (kappa[K] + kappa0) * S2[K] + q0 * TKE_decay[K]
                bQd1 = h_Int[K] * (TKE_decay[K] + dz_h_Int * N2[K] * K_Q[K]) + cQcomp * aQ[K - 1]
                bQ = 1.0 / (bQd1 + aQ[K])
                tke[K] = bQ * (h_Int[K] * tke_src + aQ[K - 1] * tke[K - 1])
                cQ[K + 1] = aQ[K] * bQ; cQcomp = bQd1 * bQ
            if ke_tke == nz + 1:
                tke[nz + 1] = TKE_min
                dQ[nz + 1] = 0.0
            else:
                br["ke_tke_interior"] += 1
                K = ke_tke
                tke_src = dz_h_Int * kappa0 * S2[K] + q0 * TKE_decay[K]
                bQ = 1.0 / ((h_Int[K] * TKE_decay[K] + cQcomp * aQ[K - 1]) + aQ[K])
                cQ[K + 1] = aQ[K] * bQ
                dQ[K] = -tke[K]
                tke[K] = fmax1((bQ * (h_Int[K] * tke_src + aQ[K - 1] * tke[K - 1]) +
                                cQ[K + 1] * (tke[K + 1] - e1[K + 1] * tke[K])) / (1.0 - cQ[K + 1] * e1[K + 1]), TKE_min)
                dQ[K] = tke[K] + dQ[K]
                K = ke_tke + 1
                while K <= nz + 1:                                   # a Fortran do loop: K is nz + 2 when it runs out
                    dQ[K] = e1[K] * dQ[K - 1]
                    tke[K] = fmax1(tke[K] + dQ[K], TKE_min)
                    if abs(dQ[K]) < roundoff * tke[K]:
                        break
                    K += 1
                for K2 in range(K + 1, nz + 1):
                    if dQ[K2] == 0.0:
                        break
                    dQ[K2] = 0.0
            for K in range(ke_tke - 1, 0, -1):
                tke[K] = fmax1(tke[K] + cQ[K + 1] * tke[K + 1], TKE_min)
                dQ[K] = tke[K] + dQ[K]

            ke_kappa_prev = ke_kappa; ks_kappa_prev = ks_kappa
            dK[1] = 0.0
            cK[2] = 0.0; cKcomp = 1.0
            if itt == 1:
                for K in range(2, nz + 1):
                    I_Ld2[K] = dz_h_Int * (N2[K] * Ilambda2 + f2) / tke[K] + I_L2_bdry[K]
            for K in range(2, nz + 1):
                dK[K] = -kappa[K]
                if itt > 1:
                    I_Ld2[K] = dz_h_Int * (N2[K] * Ilambda2 + f2) / tke[K] + I_L2_bdry[K]
                bKd1 = h_Int[K] * I_Ld2[K] + cKcomp * Idz[K - 1]
                bK = 1.0 / (bKd1 + Idz[K])
                kappa[K] = bK * (Idz[K - 1] * kappa[K - 1] + h_Int[K] * k_src[K])
                cK[K + 1] = Idz[K] * bK; cKcomp = bKd1 * bK
                if kappa[K] < cKcomp * kappa_trunc:
                    kappa[K] = 0.0
                    if K > ke_src:
                        ke_kappa = K - 1; K_Q[K] = 0.0
                        br["kappa_trunc_bottom"] += 1
                        break
                elif kappa[K] < 2.0 * cKcomp * kappa_trunc:
                    br["kappa_small_fwd"] += 1
                    kappa[K] = 2.0 * (kappa[K] - cKcomp * kappa_trunc)
            K_Q[ke_kappa] = kappa[ke_kappa] / tke[ke_kappa]
            dK[ke_kappa] = dK[ke_kappa] + kappa[ke_kappa]
            for K in range(ke_kappa + 2, ke_kappa_prev + 1):
                dK[K] = -kappa[K]; kappa[K] = 0.0; K_Q[K] = 0.0
            for K in range(ke_kappa - 1, 1, -1):
                kappa[K] = kappa[K] + cK[K + 1] * kappa[K + 1]
                if kappa[K] <= kappa_trunc:
                    kappa[K] = 0.0
                    if K < ks_src:
                        ks_kappa = K + 1; K_Q[K] = 0.0
                        br["kappa_trunc_top"] += 1
                        break
                elif kappa[K] < 2.0 * kappa_trunc:
                    br["kappa_small_bwd"] += 1
                    kappa[K] = 2.0 * (kappa[K] - kappa_trunc)
                dK[K] = dK[K] + kappa[K]
                K_Q[K] = kappa[K] / tke[K]
            for K in range(ks_kappa_prev, ks_kappa - 1):
                kappa[K] = 0.0; K_Q[K] = 0.0
        else:
            br["newton_entered"] += 1
            ks_kappa_prev = ks_kappa; ke_kappa_prev = ke_kappa; ke_kappa = nz
            ks_kappa = 2
            dK[1] = 0.0; cK[2] = 0.0; cKcomp = 1.0; dKdQ[1] = 0.0
            aQ[1] = (0.5 * (kappa[1] + kappa[2]) + kappa0) * Idz[1]
            dQdz[1] = 0.5 * (tke[1] - tke[2]) * Idz[1]
            dQ[1] = 0.0; cQ[2] = 0.0; cQcomp = 1.0; dQmdK[2] = 0.0
            for K in range(2, nz + 1):
                I_Q = 1.0 / tke[K]
                I_Ld2[K] = (N2[K] * Ilambda2 + f2) * dz_h_Int * I_Q + I_L2_bdry[K]
                kap_src = h_Int[K] * (k_src[K] - I_Ld2[K] * kappa[K]) + \
                    Idz[K - 1] * (kappa[K - 1] - kappa[K]) - Idz[K] * (kappa[K] - kappa[K + 1])
                decay_term_k = -Idz[K - 1] * dQmdK[K] * dKdQ[K - 1] + h_Int[K] * I_Ld2[K]
                if decay_term_k < 0.0:
                    abort_Newton = True; br["newton_pivot_K"] += 1
                    break
                bK = 1.0 / (Idz[K] + Idz[K - 1] * cKcomp + decay_term_k)
                cK[K + 1] = bK * Idz[K]
                cKcomp = bK * (Idz[K - 1] * cKcomp + decay_term_k)
                if CS.dKdQ_iteration_bug:
                    br["dKdQ_bug"] += 1
                    dKdQ[K] = bK * (Idz[K - 1] * dKdQ[K - 1] * cQ[K] +
                                    CS.m_to_Z * (N2[K] * Ilambda2 + f2) * (I_Q * I_Q) * kappa[K])
                else:
                    br["dKdQ_fixed"] += 1
                    dKdQ[K] = bK * (Idz[K - 1] * dKdQ[K - 1] * cQ[K] +
                                    dz_Int[K] * (N2[K] * Ilambda2 + f2) * (I_Q * I_Q) * kappa[K])
                dK[K] = bK * (kap_src + Idz[K - 1] * dK[K - 1] + Idz[K - 1] * dKdQ[K - 1] * dQ[K - 1])
                if dK[K] <= cKcomp * (kappa_trunc - kappa[K]):
                    dK[K] = -cKcomp * kappa[K]
                elif dK[K] < cKcomp * (2.0 * kappa_trunc - kappa[K]):
                    dK[K] = 2.0 * dK[K] - cKcomp * (2.0 * kappa_trunc - kappa[K])
                aQ[K] = (0.5 * (kappa[K] + kappa[K + 1]) + kappa0) * Idz[K]
                dQdz[K] = 0.5 * (tke[K] - tke[K + 1]) * Idz[K]
                tke_src = h_Int[K] * ((dz_h_Int * ((kappa[K] + kappa0) * S2[K] - kappa[K] * N2[K])) -
                                      (tke[K] - q0) * TKE_decay[K]) - \
                    (aQ[K] * (tke[K] - tke[K + 1]) - aQ[K - 1] * (tke[K - 1] - tke[K]))
                v1 = aQ[K - 1] + dQdz[K - 1] * dKdQ[K - 1]
                v2 = (v1 * dQmdK[K] + dQdz[K - 1] * cK[K]) + ((dQdz[K - 1] - dQdz[K]) + dz_Int[K] * (S2[K] - N2[K]))
                decay_term_Q = h_Int[K] * TKE_decay[K] - dQdz[K - 1] * dKdQ[K - 1] * cQ[K] - v2 * dKdQ[K]
                if decay_term_Q < 0.0:
                    abort_Newton = True; br["newton_pivot_Q"] += 1
                    break
                bQ = 1.0 / (aQ[K] + (cQcomp * aQ[K - 1] + decay_term_Q))
                cQ[K + 1] = aQ[K] * bQ
                cQcomp = (cQcomp * aQ[K - 1] + decay_term_Q) * bQ
                dQmdK[K + 1] = (v2 * cK[K + 1] - dQdz[K]) * bQ
                dQ[K] = fmax1(bQ * ((v1 * dQ[K - 1] + dQdz[K - 1] * dK[K - 1]) + (v2 * dK[K] + tke_src)), cQcomp * (-0.5 * tke[K]))
                if (itt > 1) and (K > ke_src) and (dK[K] == 0.0) and ((kappa[K] + kappa[K + 1]) == 0.0):
                    ke_kappa = K - 1; br["newton_left_early"] += 1
                    break
            if (ke_kappa == nz) and (not abort_Newton):
                dK[nz + 1] = 0.0; dKdQ[nz + 1] = 0.0
                dQ[nz + 1] = 0.0
            elif not abort_Newton:
                dQ[ke_kappa + 1] = dQ[ke_kappa + 1] / (1.0 - cQ[ke_kappa + 2] * e1[ke_kappa + 2])
                tke[ke_kappa + 1] = fmax1(tke[ke_kappa + 1] + dQ[ke_kappa + 1], TKE_min)
                for k in range(ke_kappa + 2, nz + 2):
                    dK[k] = 0.0
                    dQ[k] = fmax1(e1[k] * dQ[k - 1], -0.5 * tke[k])
                    tke[k] = fmax1(tke[k] + dQ[k], TKE_min)
                    if abs(dQ[k]) < roundoff * tke[k]:
                        break
            if not abort_Newton:
                for K in range(ke_kappa, 1, -1):
                    dQ[K] = fmax1(dQ[K] + (cQ[K + 1] * dQ[K + 1] + dQmdK[K + 1] * dK[K + 1]), -0.5 * tke[K])
                    tke[K] = fmax1(tke[K] + dQ[K], TKE_min)
                    dK[K] = dK[K] + (cK[K + 1] * dK[K + 1] + dKdQ[K] * dQ[K])
                    if dK[K] <= kappa_trunc - kappa[K]:
                        dK[K] = -kappa[K]
                        kappa[K] = 0.0
                        if (K < ks_src) and (K + 1 > ks_kappa):
                            ks_kappa = K + 1
                    elif dK[K] < 2.0 * kappa_trunc - kappa[K]:
                        dK[K] = 2.0 * dK[K] - (2.0 * kappa_trunc - kappa[K])
                        kappa[K] = fmax1(kappa[K] + dK[K], 0.0)
                        if K <= ks_kappa:
                            ks_kappa = 2
                    else:
                        kappa[K] = kappa[K] + dK[K]
                        if K <= ks_kappa:
                            ks_kappa = 2
                dQ[1] = fmax1(dQ[1] + cQ[2] * dQ[2] + dQmdK[2] * dK[2], TKE_min - tke[1])
                tke[1] = fmax1(tke[1] + dQ[1], TKE_min)
                dK[1] = 0.0

        if (tol_err < Newton_err) and (not abort_Newton):
            Newton_test = Newton_err
            if do_Newton:
                Newton_test = 2.0 * Newton_err
            within_tolerance = True; do_Newton = True
            for K in range(min(ks_kappa, ks_kappa_prev), max(ke_kappa, ke_kappa_prev) + 1):
                kappa_mean = kappa0 + (kappa[K] - 0.5 * dK[K])
                if abs(dK[K]) > Newton_test * kappa_mean:
                    if do_Newton:
                        abort_Newton = True
                    within_tolerance = False; do_Newton = False
                    break
                elif abs(dK[K]) > tol_err * kappa_mean:
                    within_tolerance = False
                    if not do_Newton:
                        break
                if abs(dQ[K]) > Newton_test * (tke[K] - 0.5 * dQ[K]):
                    if do_Newton:
                        abort_Newton = True
                    do_Newton = False
                    if not within_tolerance:
                        break
        else:
            within_tolerance = True
            for K in range(min(ks_kappa, ks_kappa_prev), max(ke_kappa, ke_kappa_prev) + 1):
                if abs(dK[K]) > tol_err * (kappa0 + (kappa[K] - 0.5 * dK[K])):
                    within_tolerance = False
                    break
        if abort_Newton:
            br["newton_aborted"] += 1
            do_Newton = False; abort_Newton = False
            Newton_err = 0.5 * Newton_err
            ke_kappa_prev = nz
            for K in range(2, nz + 1):
                K_Q[K] = kappa[K] / fmax1(tke[K], TKE_min)
        if within_tolerance:
            break
    else:
        br["itt_limit"] += 1

    if do_Newton:
        br["newton_K_Q"] += 1
        for K in range(1, ks_kappa):
            K_Q[K] = 0.0
        for K in range(ks_kappa, ke_kappa + 1):
            K_Q[K] = kappa[K] / tke[K]
        for K in range(ke_kappa + 1, nz + 2):
            K_Q[K] = 0.0
    if local_src is not None:
        local_src[1] = 0.0; local_src[nz + 1] = 0.0
        for K in range(2, nz + 1):
            diffusive_src = Idz[K - 1] * (kappa[K - 1] - kappa[K]) + Idz[K] * (kappa[K + 1] - kappa[K])
            chg_by_k0 = kappa0 * ((Idz[K - 1] + Idz[K]) / h_Int[K] + I_Ld2[K])
            if diffusive_src <= 0.0:
                local_src[K] = k_src[K] + chg_by_k0
            else:
                local_src[K] = (k_src[K] + chg_by_k0) + diffusive_src / h_Int[K]
    if kappa_src is not None:
        kappa_src[1] = 0.0; kappa_src[nz + 1] = 0.0
        for K in range(2, nz + 1):
            kappa_src[K] = k_src[K]
    return its


def kappa_shear_column(CS, GV, nk, kappa, dt, nzc, f2, surface_pres, hlay, dz_lay, u0xdz, v0xdz, T0xdz, S0xdz, use_temperature,
                       derivs, br):
    """:864-1372.  kappa: the first guess, nzc + 1 values from index 1.  derivs(T_int, Sal_int, pressure) gives dRho_dT, dRho_dS of
    lists of points [kg m-3 degC-1, kg m-3 ppt-1] at RL2_T2_to_Pa times the pressure.  Returns a dict of the column's results
    (lists indexed from 1) and `its`, the outer iterations made."""
    n2 = nzc + 2
    new = lambda: [NAN] * n2                                          # noqa: E731
    u = new(); v = new(); Idz = new(); T = new(); Sal = new(); u_test = new(); v_test = new(); T_test = new(); S_test = new()
    N2 = new(); h_Int = new(); dz_Int = new(); I_dz_int = new(); S2 = new(); a1 = new(); c1 = new()
    kappa_src = new(); kappa_out = new(); kappa_mid = new(); tke = new(); tke_pred = new(); kappa_pred = new(); pressure = new()
    T_int = new(); Sal_int = new(); dbuoy_dT = new(); dbuoy_dS = new(); I_L2_bdry = new(); K_Q = new(); K_Q_tmp = new()
    local_src_avg = new(); tol_min = new(); tol_max = new(); tol_chg = new(); dist_from_top = new(); h_from_top = new()
    local_src = new(); kappa_avg = new(); tke_avg = new(); N2_mean = new(); S2_mean = new(); N2_init = new(); S2_init = new()

    Ri_crit = CS.RiNo_crit
    gR0 = GV.H_to_RZ * GV.g_Earth
    g_R0 = CS.g_Earth_Z_T2 / GV.Rho0
    k0dt = dt * CS.kappa_0
    I_lz_rescale_sqr = 1.0
    if CS.lz_rescale > 0:
        I_lz_rescale_sqr = 1 / (CS.lz_rescale * CS.lz_rescale)
        if CS.lz_rescale != 1.0:
            br["lz_rescale"] += 1
    tol_dksrc = CS.kappa_src_max_chg
    if tol_dksrc == 10.0:
        tol_dksrc_low = 0.95
    else:
        tol_dksrc_low = (tol_dksrc - 0.5) / tol_dksrc
    tol2 = 2.0 * CS.kappa_tol_err
    dt_refinements = 5
    dz_h_Int = GV.H_to_Z                                             # :1110, Boussinesq
    L_to_Z = CS.L_to_Z
    vel_under = CS.vel_underflow

    for k in range(1, nzc + 1):
        Idz[k] = 1.0 / dz_lay[k]
    I_dz_int[1] = 2.0 / dz_lay[1]
    dist_from_top[1] = 0.0; h_from_top[1] = 0.0
    for K in range(2, nzc + 1):
        I_dz_int[K] = 2.0 / (dz_lay[K - 1] + dz_lay[K])
        dist_from_top[K] = dist_from_top[K - 1] + dz_lay[K - 1]
        h_from_top[K] = h_from_top[K - 1] + hlay[K - 1]
    I_dz_int[nzc + 1] = 2.0 / dz_lay[nzc]
    dist_from_bot = 0.0; h_from_bot = 0.0
    for K in range(nzc, 1, -1):
        dist_from_bot = dist_from_bot + dz_lay[K]
        h_from_bot = h_from_bot + hlay[K]
        I_L2_bdry[K] = ((dist_from_top[K] + dist_from_bot) * (h_from_top[K] + h_from_bot)) / \
            ((dist_from_top[K] * dist_from_bot) * (h_from_top[K] * h_from_bot))
        I_L2_bdry[K] = I_lz_rescale_sqr * I_L2_bdry[K]

    if nzc > 1:
        a1[2] = k0dt * I_dz_int[2]
        b1 = 1.0 / (hlay[1] + a1[2])
        u[1] = b1 * u0xdz[1]; v[1] = b1 * v0xdz[1]
        T[1] = b1 * T0xdz[1]; Sal[1] = b1 * S0xdz[1]
        c1[2] = a1[2] * b1; d1 = hlay[1] * b1
        for k in range(2, nzc):
            bd1 = hlay[k] + d1 * a1[k]
            a1[k + 1] = k0dt * I_dz_int[k + 1]
            b1 = 1.0 / (bd1 + a1[k + 1])
            u[k] = b1 * (u0xdz[k] + a1[k] * u[k - 1])
            v[k] = b1 * (v0xdz[k] + a1[k] * v[k - 1])
            T[k] = b1 * (T0xdz[k] + a1[k] * T[k - 1])
            Sal[k] = b1 * (S0xdz[k] + a1[k] * Sal[k - 1])
            c1[k + 1] = a1[k + 1] * b1; d1 = bd1 * b1
        b1 = 1.0 / ((hlay[nzc] + d1 * a1[nzc]) + k0dt * I_dz_int[nzc + 1])
        u[nzc] = b1 * (u0xdz[nzc] + a1[nzc] * u[nzc - 1])
        v[nzc] = b1 * (v0xdz[nzc] + a1[nzc] * v[nzc - 1])
        b1 = 1.0 / (hlay[nzc] + d1 * a1[nzc])
        T[nzc] = b1 * (T0xdz[nzc] + a1[nzc] * T[nzc - 1])
        Sal[nzc] = b1 * (S0xdz[nzc] + a1[nzc] * Sal[nzc - 1])
        for k in range(nzc - 1, 0, -1):
            u[k] = u[k] + c1[k + 1] * u[k + 1]; v[k] = v[k] + c1[k + 1] * v[k + 1]
            T[k] = T[k] + c1[k + 1] * T[k + 1]; Sal[k] = Sal[k] + c1[k + 1] * Sal[k + 1]
    else:
        br["nzc_1"] += 1
        b1 = 1.0 / (hlay[1] + k0dt * I_dz_int[2])
        u[1] = b1 * u0xdz[1]; v[1] = b1 * v0xdz[1]
        b1 = 1.0 / hlay[1]
        T[1] = b1 * T0xdz[1]; Sal[1] = b1 * S0xdz[1]

    h_Int[1] = 0.0; h_Int[2] = hlay[1]
    dz_Int[1] = 0.0; dz_Int[2] = dz_lay[1]
    for K in range(2, nzc):
        Norm = 1.0 / (hlay[K] * (hlay[K - 1] + hlay[K + 1]) + 2.0 * hlay[K - 1] * hlay[K + 1])
        wt_a = ((hlay[K] + hlay[K + 1]) * hlay[K - 1]) * Norm
        wt_b = ((hlay[K - 1] + hlay[K]) * hlay[K + 1]) * Norm
        h_Int[K] = h_Int[K] + hlay[K] * wt_a
        h_Int[K + 1] = hlay[K] * wt_b
        dz_Int[K] = dz_Int[K] + dz_lay[K] * wt_a
        dz_Int[K + 1] = dz_lay[K] * wt_b
    h_Int[nzc] = h_Int[nzc] + hlay[nzc]; h_Int[nzc + 1] = 0.0
    dz_Int[nzc] = dz_Int[nzc] + dz_lay[nzc]; dz_Int[nzc + 1] = 0.0

    if use_temperature:
        br["eos"] += 1
        pressure[1] = surface_pres
        for K in range(2, nzc + 1):
            pressure[K] = pressure[K - 1] + gR0 * hlay[K - 1]
            T_int[K] = 0.5 * (T[K - 1] + T[K])
            Sal_int[K] = 0.5 * (Sal[K - 1] + Sal[K])
        if nzc >= 2:
            dT, dS = derivs(T_int[2:nzc + 1], Sal_int[2:nzc + 1], [CS.RL2_T2_to_Pa * p for p in pressure[2:nzc + 1]])
            rho_scale = CS.kg_m3_to_R * (-g_R0)                      # MOM_EOS.F90:820-827 with C_to_degC = S_to_ppt = 1
            for K in range(2, nzc + 1):
                dbuoy_dT[K] = rho_scale * dT[K - 2]
                dbuoy_dS[K] = rho_scale * dS[K - 2]
    else:
        br["layered"] += 1
        for K in range(1, nzc + 2):
            dbuoy_dT[K] = -g_R0; dbuoy_dS[K] = 0.0

    calculate_projected_state(kappa, u, v, T, Sal, 0.0, nzc, hlay, I_dz_int, dbuoy_dT, dbuoy_dS, vel_under, u, v, T, Sal, N2, S2,
                              L_to_Z, br)
    for K in range(1, nzc + 2):
        N2_init[K] = N2[K]
        S2_init[K] = S2[K]

    dt_rem = dt
    for K in range(1, nzc + 2):
        K_Q[K] = 0.0
        kappa_avg[K] = 0.0; tke_avg[K] = 0.0; N2_mean[K] = 0.0; S2_mean[K] = 0.0
        local_src_avg[K] = 0.0
        if h_Int[K] > 0.0:
            local_src_avg[K] = 0.1 * k0dt * I_dz_int[K] / h_Int[K]

    its = 0
    first_tke = None
    for itt in range(1, CS.max_KS_it + 1):
        its = itt
        find_kappa_tke(CS, N2, S2, kappa, Idz, h_Int, dz_Int, dz_h_Int, I_L2_bdry, f2, nzc, K_Q, tke, kappa_out, br,
                       kappa_src=kappa_src, local_src=local_src)
        if itt == 1:
            first_tke = list(tke)
        ks_kappa = nk + 1; ke_kappa = 0
        for K in range(2, nzc + 1):
            if kappa_out[K] > 0.0:
                ks_kappa = K
                break
        for K in range(nzc, ks_kappa - 1, -1):
            if kappa_out[K] > 0.0:
                ke_kappa = K
                break
        if ke_kappa == nzc:
            kappa_out[nzc + 1] = 0.0

        if (ke_kappa < ks_kappa) or (itt == CS.max_KS_it):
            if not (ke_kappa < ks_kappa):
                br["last_iteration"] += 1
            dt_now = dt_rem
        else:
            dt_test = dt_rem
            for K in range(2, nzc + 1):
                tol_max[K] = kappa_src[K] + tol_dksrc * local_src[K]
                tol_min[K] = kappa_src[K] - tol_dksrc_low * local_src[K]
                tol_chg[K] = tol2 * local_src_avg[K]
            valid_dt = None
            for itt_dt in range(1, (CS.max_KS_it + 1 - itt) // 2 + 1):
                calculate_projected_state(kappa_out, u, v, T, Sal, 0.5 * dt_test, nzc, hlay, I_dz_int, dbuoy_dT, dbuoy_dS, vel_under,
                                          u_test, v_test, T_test, S_test, N2, S2, L_to_Z, br, ks_int=ks_kappa, ke_int=ke_kappa)
                valid_dt = True
                Idtt = 1.0 / dt_test
                for K in range(max(ks_kappa - 1, 2), min(ke_kappa + 1, nzc) + 1):
                    if N2[K] < Ri_crit * S2[K]:
                        K_src = (2.0 * CS.Shearmix_rate * math.sqrt(S2[K])) * \
                            ((Ri_crit * S2[K] - N2[K]) / (Ri_crit * S2[K] + CS.FRi_curvature * N2[K]))
                        if CS.restrictive_tolerance_check:
                            br["tol_restrictive"] += 1
                            if (K_src > fmin1(tol_max[K], kappa_src[K] + Idtt * tol_chg[K])) or \
                               (K_src < fmax1(tol_min[K], kappa_src[K] - Idtt * tol_chg[K])):
                                valid_dt = False
                                break
                        else:
                            br["tol_loose"] += 1
                            if (K_src > fmax1(tol_max[K], kappa_src[K] + Idtt * tol_chg[K])) or \
                               (K_src < fmin1(tol_min[K], kappa_src[K] - Idtt * tol_chg[K])):
                                valid_dt = False
                                break
                    else:
                        br["scan_stable_arm"] += 1
                        if 0.0 < fmin1(tol_min[K], kappa_src[K] - Idtt * tol_chg[K]):
                            br["scan_stable_invalid"] += 1
                            valid_dt = False
                            break
                if valid_dt:
                    break
                br["halved"] += 1
                dt_test = 0.5 * dt_test
            if not valid_dt:
                br["halving_ran_out"] += 1
            if (dt_test < dt_rem) and valid_dt:
                dt_inc = 0.5 * dt_test
                for itt_dt in range(1, dt_refinements + 1):
                    calculate_projected_state(kappa_out, u, v, T, Sal, 0.5 * (dt_test + dt_inc), nzc, hlay, I_dz_int, dbuoy_dT,
                                              dbuoy_dS, vel_under, u_test, v_test, T_test, S_test, N2, S2, L_to_Z, br,
                                              ks_int=ks_kappa, ke_int=ke_kappa)
                    valid_dt = True
                    Idtt = 1.0 / (dt_test + dt_inc)
                    for K in range(max(ks_kappa - 1, 2), min(ke_kappa + 1, nzc) + 1):
                        if N2[K] < Ri_crit * S2[K]:
                            K_src = (2.0 * CS.Shearmix_rate * math.sqrt(S2[K])) * \
                                ((Ri_crit * S2[K] - N2[K]) / (Ri_crit * S2[K] + CS.FRi_curvature * N2[K]))
                            if (K_src > fmax1(tol_max[K], kappa_src[K] + Idtt * tol_chg[K])) or \
                               (K_src < fmin1(tol_min[K], kappa_src[K] - Idtt * tol_chg[K])):
                                valid_dt = False
                                break
                        else:
                            if 0.0 < fmin1(tol_min[K], kappa_src[K] - Idtt * tol_chg[K]):
                                valid_dt = False
                                break
                    if valid_dt:
                        br["refine_accept"] += 1
                        dt_test = dt_test + dt_inc
                    else:
                        br["refine_reject"] += 1
                    dt_inc = 0.5 * dt_inc
            else:
                dt_inc = 0.0
            dt_now = fmin1(dt_test * (1.0 + CS.kappa_tol_err) + dt_inc, dt_rem)
            for K in range(2, nzc + 1):
                local_src_avg[K] = local_src_avg[K] + dt_now * local_src[K]

        if ke_kappa < ks_kappa:
            br["no_mixing_exit"] += 1
            dt_wt = dt_rem / dt; dt_rem = 0.0
            for K in range(1, nzc + 2):
                kappa_mid[K] = 0.0
                tke_avg[K] = tke_avg[K] + dt_wt * tke[K]
        else:
            br["pred_corr"] += 1
            calculate_projected_state(kappa_out, u, v, T, Sal, dt_now, nzc, hlay, I_dz_int, dbuoy_dT, dbuoy_dS, vel_under,
                                      u_test, v_test, T_test, S_test, N2, S2, L_to_Z, br, ks_int=ks_kappa, ke_int=ke_kappa)
            for K in range(1, nzc + 2):
                K_Q_tmp[K] = K_Q[K]
            find_kappa_tke(CS, N2, S2, kappa_out, Idz, h_Int, dz_Int, dz_h_Int, I_L2_bdry, f2, nzc, K_Q_tmp, tke_pred, kappa_pred, br)
            ks_kappa = nk + 1; ke_kappa = 0
            for K in range(1, nzc + 2):
                kappa_mid[K] = 0.5 * (kappa_out[K] + kappa_pred[K])
                if (kappa_mid[K] > 0.0) and (K < ks_kappa):
                    ks_kappa = K
                if kappa_mid[K] > 0.0:
                    ke_kappa = K
            calculate_projected_state(kappa_mid, u, v, T, Sal, dt_now, nzc, hlay, I_dz_int, dbuoy_dT, dbuoy_dS, vel_under,
                                      u_test, v_test, T_test, S_test, N2, S2, L_to_Z, br, ks_int=ks_kappa, ke_int=ke_kappa)
            find_kappa_tke(CS, N2, S2, kappa_out, Idz, h_Int, dz_Int, dz_h_Int, I_L2_bdry, f2, nzc, K_Q, tke_pred, kappa_pred, br)
            dt_wt = dt_now / dt; dt_rem = dt_rem - dt_now
            for K in range(1, nzc + 2):
                kappa_mid[K] = 0.5 * (kappa_out[K] + kappa_pred[K])
                kappa_avg[K] = kappa_avg[K] + kappa_mid[K] * dt_wt
                tke_avg[K] = tke_avg[K] + dt_wt * 0.5 * (tke_pred[K] + tke[K])
                N2_mean[K] = N2_mean[K] + dt_wt * N2[K]
                S2_mean[K] = S2_mean[K] + dt_wt * S2[K]
                kappa[K] = kappa_pred[K]
        if dt_rem > 0.0:
            calculate_projected_state(kappa_mid, u, v, T, Sal, dt_now, nzc, hlay, I_dz_int, dbuoy_dT, dbuoy_dS, vel_under,
                                      u, v, T, Sal, N2, S2, L_to_Z, br)
        if dt_rem <= 0.0:
            break
    if its >= 2:
        br["two_iterations"] += 1
    return dict(kappa_avg=kappa_avg, tke=tke, tke_avg=tke_avg, N2_init=N2_init, S2_init=S2_init, N2_mean=N2_mean, S2_mean=S2_mean,
                first_tke=first_tke), its


def Calculate_kappa_shear(d, M, GV, CS, eos, u, v, h, T, S, p_surf, dt, zero_mix, kappa_io, tke_io, kv_io, Rlay=None, orc=None,
                          counts=None, traces=None, **diag):
    """The driver's find_uv_at_h (MOM_diabatic_driver.F90:1391-1398) and Calculate_kappa_shear :133-411 on the arrays of a tile.
    kappa_io, tke_io, kv_io and the diagnostics given by name are written on the computational domain.  T and S both None: the
    layered arm with Rlay.  traces: a dict that gets {(j, i): (nzc, its, first_tke)} of the wet columns."""
    br = counts if counts is not None else new_counts()
    nz = d.nk
    assert set(diag) <= set(DIAG_3D + DIAG_2D), sorted(diag)
    use_temperature = T is not None
    assert (T is None) == (S is None)
    assert use_temperature or Rlay is not None
    u_h, v_h = find_uv_at_h(d, M, GV, u, v, h, zero_mix, br)
    k0dt = dt * CS.kappa_0
    dz_massless = 0.1 * math.sqrt(CS.Z_to_m_m_to_H * k0dt)
    mask = M[G["mask2dT"]]; f2B = M[G["Coriolis2Bu"]]

    def derivs(Ti, Si, pi):
        a, b = _derivs(orc, eos, np.array(Ti), np.array(Si), np.array(pi))
        return a.tolist(), b.tolist()

    for jl in range(d.nj):
        for il in range(d.ni):
            j = jl + d.joff; i = il + d.ioff
            if not (mask[j, i] > 0.0):
                br["land"] += 1
                kappa_io[:, j, i] = float(mask[j, i]) * 0.0
                tke_io[:, j, i] = float(mask[j, i]) * 0.0
                kv_io[:, j, i] = (float(mask[j, i]) * 0.0) * CS.Prandtl_turb
                for n in diag:
                    diag[n][..., j, i] = 0.0
                continue
            h_2d = [NAN] + [float(x) for x in h[:, j, i]]
            dz_2d = [NAN] + [GV.H_to_Z * float(x) for x in h[:, j, i]]      # thickness_to_dz, Boussinesq
            u_2d = [NAN] + [float(x) for x in u_h[:, j, i]]
            v_2d = [NAN] + [float(x) for x in v_h[:, j, i]]
            if use_temperature:
                T_2d = [NAN] + [float(x) for x in T[:, j, i]]
                S_2d = [NAN] + [float(x) for x in S[:, j, i]]
            else:
                T_2d = S_2d = [NAN] + [float(x) for x in Rlay]
            n2 = nz + 2
            h_lay = [NAN] * n2; dz_lay = [NAN] * n2; u0xdz = [NAN] * n2; v0xdz = [NAN] * n2; T0xdz = [NAN] * n2; S0xdz = [NAN] * n2
            kc = [0] * n2; kf = [NAN] * n2
            if CS.eliminate_massless:
                br["elim_on"] += 1
                if CS.nkml > 1:
                    br["nkml_gt1"] += 1
                nzc = 1
                for k in range(1, nz + 1):
                    h_lay[k] = 0.0; dz_lay[k] = 0.0; u0xdz[k] = 0.0; v0xdz[k] = 0.0
                    T0xdz[k] = 0.0; S0xdz[k] = 0.0
                    if (k > CS.nkml) and (h_lay[nzc] > 0.0) and (h_2d[k] > dz_massless):
                        nzc = nzc + 1
                    kc[k] = nzc
                    h_lay[nzc] = h_lay[nzc] + h_2d[k]
                    dz_lay[nzc] = dz_lay[nzc] + dz_2d[k]
                    u0xdz[nzc] = u0xdz[nzc] + u_2d[k] * h_2d[k]
                    v0xdz[nzc] = v0xdz[nzc] + v_2d[k] * h_2d[k]
                    T0xdz[nzc] = T0xdz[nzc] + T_2d[k] * h_2d[k]
                    S0xdz[nzc] = S0xdz[nzc] + S_2d[k] * h_2d[k]
                kc[nz + 1] = nzc + 1
                Idz = [NAN] * n2
                for k in range(1, nzc + 1):
                    Idz[k] = 1.0 / h_lay[k]
                kf[1] = 0.0; dz_in_lay = h_2d[1]
                for k in range(2, nz + 1):
                    if kc[k] > kc[k - 1]:
                        kf[k] = 0.0; dz_in_lay = h_2d[k]
                    else:
                        kf[k] = dz_in_lay * Idz[kc[k]]; dz_in_lay = dz_in_lay + h_2d[k]
                kf[nz + 1] = 0.0
            else:
                br["elim_off"] += 1
                for k in range(1, nz + 1):
                    h_lay[k] = h_2d[k]
                    dz_lay[k] = dz_2d[k]
                    u0xdz[k] = u_2d[k] * h_lay[k]; v0xdz[k] = v_2d[k] * h_lay[k]
                    T0xdz[k] = T_2d[k] * h_lay[k]; S0xdz[k] = S_2d[k] * h_lay[k]
                nzc = nz
                for k in range(1, nzc + 2):
                    kc[k] = k; kf[k] = 0.0
            f2 = 0.25 * ((float(f2B[j, i]) + float(f2B[j - 1, i - 1])) + (float(f2B[j - 1, i]) + float(f2B[j, i - 1])))
            surface_pres = 0.0
            if p_surf is not None:
                surface_pres = float(p_surf[j, i])
            kappa = [NAN] + [CS.kappa_seed] * (nzc + 1)
            col, its = kappa_shear_column(CS, GV, nz, kappa, dt, nzc, f2, surface_pres, h_lay, dz_lay, u0xdz, v0xdz, T0xdz, S0xdz,
                                          use_temperature, derivs, br)
            if traces is not None:
                traces[(jl, il)] = (nzc, its, col["first_tke"])
            kappa_2d = [NAN] * n2; tke_2d = [NAN] * n2
            dg = {n: [NAN] * n2 for n in DIAG_3D}
            if nz == nzc:
                br["all_layer_bug" if CS.all_layer_TKE_bug else "all_layer_avg"] += 1
                for K in range(1, nz + 2):
                    kappa_2d[K] = col["kappa_avg"][K]
                    tke_2d[K] = col["tke"][K] if CS.all_layer_TKE_bug else col["tke_avg"][K]
                    for n in DIAG_3D:
                        dg[n][K] = col[n][K]
            else:
                br["merged"] += 1
                anyf = False
                for K in range(1, nz + 2):
                    c = kc[K]
                    if kf[K] == 0.0:
                        kappa_2d[K] = col["kappa_avg"][c]
                        tke_2d[K] = col["tke_avg"][c]
                        for n in DIAG_3D:
                            dg[n][K] = col[n][c]
                    else:
                        anyf = True
                        kappa_2d[K] = (1.0 - kf[K]) * col["kappa_avg"][c] + kf[K] * col["kappa_avg"][c + 1]
                        tke_2d[K] = (1.0 - kf[K]) * col["tke_avg"][c] + kf[K] * col["tke_avg"][c + 1]
                        for n in DIAG_3D:
                            dg[n][K] = (1.0 - kf[K]) * col[n][c] + kf[K] * col[n][c + 1]
                if anyf:
                    br["kf_pos"] += 1
            mk = float(mask[j, i])
            for K in range(1, nz + 2):
                kappa_io[K - 1, j, i] = mk * kappa_2d[K]
                tke_io[K - 1, j, i] = mk * tke_2d[K]
                kv_io[K - 1, j, i] = (mk * kappa_2d[K]) * CS.Prandtl_turb
            for n in diag:
                if n == "KS_its":
                    diag[n][j, i] = float(its)
                else:
                    diag[n][:, j, i] = dg[n][1:nz + 2]
    return br


# ------------------------------------------------------------------------------------------------------------------------------
# Shared cases of tests/test_kappa_shear_cpu.py and tests/test_kappa_shear_gpu.py

def _ij(d):
    il = (np.arange(d.pitch) - d.ioff + d.i_glob0)[None, :] * np.ones(d.shape2(), int)
    jl = (np.arange(d.shape2()[0]) - d.joff + d.j_glob0)[:, None] * np.ones(d.shape2(), int)
    return il, jl


def inputs(d, M, GV, seed=5, band=0.15, U0=0.5, thin=True, zero_uv=False, p_surf=True, h0=10.0, uniform=False):
    """u, v, h, T, S, p_surf and GV%Rlay on a tile, laid in global coordinates.  Layers of about 10 m whatever their number; T falls
    by 0.5 degC and S rises by 0.02 from layer to layer (stable), Rlay rises by 0.1 kg m-3.  u is a tanh shear layer of three
    layers' width across the middle of the column, of amplitude U0*(0.6 + 0.8*smooth) in a band of rows (the fraction `band` of
    the basin, from a quarter of the way up) and a twentieth of that elsewhere; v is -0.3 times a shifted copy: the bulk Ri across
    the middle is 0.1 to 0.3 in the band and above 25 outside.  thin: some columns have layers of exactly zero thickness, others a
    layer of 0.1 mm in the shear layer (massless: below dz_massless, merged with weight kf > 0).  zero_uv: u = v = 0.  h0: the layer
    thickness in place of 10 m.  uniform: every wet layer is exactly h0 thick, T = 16 and S = 32 everywhere (with h0 a power of two
    and kappa_0 = 0 the differences of T and of S between layers are exact zeros)."""
    from mom6_amd import synth
    nk = d.nk
    il, jl = _ij(d)
    sf = lambda n, **kw: synth.smooth_field(d, seed + n, ox=0.5, oy=0.5, **kw)   # noqa: E731
    wetp = M[G["mask2dT"]] > 0.0
    h = np.stack([h0 * (1.0 + 0.3 * sf(k % 5)) for k in range(nk)])
    if thin and nk > 2:
        h[nk - 2] = np.where(il % 7 == 3, 0.0, h[nk - 2])
        h[1] = np.where(il % 13 == 5, 0.0, h[1])
        h[nk // 2] = np.where(il % 11 == 2, 1.0e-4, h[nk // 2])
    if uniform:
        h = np.full_like(h, h0)
    h = np.where(wetp, h, 0.0)
    j0 = int(0.25 * d.nj_glob); j1 = j0 + max(int(round(band * d.nj_glob)), 1)
    inband = (jl >= j0) & (jl < j1)
    amp = U0 * (0.6 + 0.8 * sf(20)) * np.where(inband, 1.0, 0.05)
    ampv = -0.3 * U0 * (0.6 + 0.8 * sf(21)) * np.where(inband, 1.0, 0.05)
    u = np.stack([amp * np.tanh((k - 0.5 * (nk - 1)) / 1.5) + 0.01 * sf(30 + k % 3) for k in range(nk)]) * M[G["mask2dCu"]]
    v = np.stack([ampv * np.tanh((k - 0.5 * (nk - 1) + 0.5) / 1.5) + 0.01 * sf(33 + k % 3) for k in range(nk)]) * M[G["mask2dCv"]]
    if zero_uv:
        u = np.zeros_like(u); v = np.zeros_like(v)
    pT, pS = sf(10), sf(11)
    T = np.stack([20.0 - 0.5 * k + 0.2 * pT for k in range(nk)])
    S = np.stack([34.5 + 0.02 * k + 0.05 * pS for k in range(nk)])
    if uniform:
        T = np.full_like(T, 16.0); S = np.full_like(S, 32.0)
    out = dict(u=u, v=v, h=h, T=T, S=S)
    if p_surf:
        out["p_surf"] = 1.0e4 * (1.0 + 0.5 * sf(40))
    out = {n: np.ascontiguousarray(a, dtype=np.float64) for n, a in out.items()}
    out["Rlay"] = np.array([1025.0 + 0.1 * k for k in range(nk)])
    return out


_ALL_DIAG = DIAG_3D + DIAG_2D
# case -> (params members, options).  Options: eos (an EOS form, None: the layered arm), zero_mix, diag (the nullable outputs handed
# in), dt, inp (keyword arguments of inputs()), eos_mods (members of the equation of state's parameters)
CASES = {
    "shear": (dict(kappa_0=1.5e-5), dict(zero_mix=True, diag=_ALL_DIAG, inp=dict(band=0.45, U0=0.8))),
    "plain_linear": (dict(restrictive_tolerance_check=1), dict(eos=abi.LINEAR, diag=("KS_its", "N2_init"), inp=dict(p_surf=False))),
    "its2": (dict(max_KS_it=2, Prandtl_turb=2.0), dict(zero_mix=True, diag=("KS_its",))),
    "bugs": (dict(dKdQ_iteration_bug=1, all_layer_TKE_bug=1, kappa_src_max_chg=5.0, lz_rescale=0.5, TKE_bg=1.0e-9, kappa_tol_err=0.02),
             dict(diag=("KS_its", "S2_mean"))),
    "elim_off": (dict(eliminate_massless=0), dict(zero_mix=True, diag=("KS_its",), inp=dict(thin=False))),
    "nkml2": (dict(nkml=2, vel_underflow=2.0e-3), dict(diag=("KS_its", "S2_init"))),
    "layered": (dict(kappa_0=1.5e-5), dict(eos=None, zero_mix=True, diag=_ALL_DIAG)),
    "quiet": (dict(), dict(zero_mix=True, diag=("KS_its",), inp=dict(U0=0.02))),
    "short_dt": (dict(max_RiNo_it=3, kappa_tol_err=0.3), dict(diag=("KS_its",), dt=300.0)),
    # a tight tolerance keeps find_kappa_tke iterating: Newton's method is entered often, and leaves on a negative pivot (:1888)
    "newton": (dict(kappa_tol_err=0.01), dict(eos=None, diag=("KS_its",), inp=dict(U0=0.8, band=0.1))),
    # no stratification at all under a linear equation of state whose density rises with T and with S, and no background
    # diffusion: dbuoy_dT*(+0) + dbuoy_dS*(+0) is -0.0 at every interior interface, and N2 = MAX(0.0, -0.0) (:1492-1502) is a tie
    "tie": (dict(kappa_0=0.0), dict(eos=abi.LINEAR, eos_mods=dict(dRho_dT=0.25, dRho_dS=0.75), diag=("KS_its", "N2_init", "N2_mean"),
                                    inp=dict(uniform=True, h0=8.0, thin=False))),
}


def case(name, GV):
    """(params, options)"""
    mods, opt = CASES[name]
    opt = dict(dict(eos=abi.WRIGHT, eos_mods={}, zero_mix=False, diag=(), dt=3600.0, inp={}), **opt)
    return abi.kappa_shear_params_default(GV, **mods), opt


def case_eos(opt):
    if opt["eos"] is None:
        return None
    eos = abi.eos_params_default(opt["eos"])
    for n, v in opt.get("eos_mods", {}).items():
        setattr(eos, n, v)
    return eos


def case_inputs(d, M, GV, opt, **kw):
    return inputs(d, M, GV, **dict(opt["inp"], **kw))


def outputs(d, opt, fill=np.nan):
    out = dict(kappa_io=np.full(d.shape3(d.nk + 1), fill), tke_io=np.full(d.shape3(d.nk + 1), fill),
               kv_io=np.full(d.shape3(d.nk + 1), fill))
    for n in opt["diag"]:
        out[n] = np.full(d.shape3(d.nk + 1) if n in DIAG_3D else d.shape2(), fill)
    return out


def run(d, M, GV, P, opt, inp, fill=np.nan, orc=None, counts=None, traces=None):
    """Calculate_kappa_shear of a case.  Returns (outputs by name, counts)."""
    counts = counts if counts is not None else new_counts()
    out = outputs(d, opt, fill)
    layered = opt["eos"] is None
    if orc is None and not layered:
        from oracle import orc as _orc
        _orc.build()
        orc = _orc
    Calculate_kappa_shear(d, M, GV, P, case_eos(opt), inp["u"], inp["v"], inp["h"], None if layered else inp["T"],
                          None if layered else inp["S"], inp.get("p_surf"), opt["dt"], opt["zero_mix"],
                          Rlay=inp["Rlay"] if layered else None, orc=orc, counts=counts, traces=traces, **out)
    return out, counts


def init_check(P, GV):
    """What mom6x_kappa_shear_init decides from the parameters alone: NotImplementedError for what the device does not carry,
    ValueError for what no run can use."""
    if P.KS_at_vertex:
        raise NotImplementedError("VERTEX_SHEAR")
    if not GV.Boussinesq:
        raise NotImplementedError("non-Boussinesq mode")
    if P.max_KS_it < 1 or P.max_RiNo_it < 1:
        raise ValueError("iteration counts")
    if not (P.RiNo_crit > 0.0):
        raise ValueError("RINO_CRIT")
    if not (P.kappa_src_max_chg > 1.0):
        raise ValueError("KAPPA_SHEAR_MAX_KAP_SRC_CHG")
    if P.work_columns < 0 or P.nkml < 1 or P.lambda_ == 0.0:
        raise ValueError("work_columns, nkml or lambda")
