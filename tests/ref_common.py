"""What the numpy restatements of the lateral modules (tests/setvisc_ref.py, thickdiff_ref.py, hordiff_ref.py, varmix_ref.py) have
in common: the reference compiler's MAX and MIN, the face ranges, the oracle's density derivatives over an array, find_eta
(src/core/MOM_interface_heights.F90:91-97), the pressure at the interfaces and vert_fill_TS
(src/core/MOM_isopycnal_slopes.F90:612-700).  Arrays are in the pitched tile layout of include/mom6x.h ([k, j + joff, i + ioff]).

The slope arithmetic is NOT here: thickdiff_ref.thickness_diffuse and varmix_ref.calc_isoneutral_slopes each restate it from their
own Fortran lines, and both check the one device function (isoneutral_grads) that the two kernels share."""
import numpy as np

from mom6_amd import abi

G = abi.G


def _max(a, b):
    """Fortran MAX(a, b): a on a tie, which decides the sign of a zero (fmax1 on the device)."""
    return np.where(b > a, b, a)


def _min(a, b):
    """Fortran MIN(a, b): a on a tie (fmin1 on the device)."""
    return np.where(b < a, b, a)


def _dmax(a, b):
    """MAX(a, b) as the compiled reference evaluates it where a tie shows: b on a tie (dmax on the device)."""
    return np.where(a > b, a, b)


def _dmin(a, b):
    """MIN(a, b) likewise: b on a tie (dmin on the device)."""
    return np.where(a < b, a, b)


def _faces(d, dir):
    """Row and column ranges of the faces (u: I = isc-1..iec, j = jsc..jec; v: i = isc..iec, J = jsc-1..jec) and the offset of
    the cell on the far side."""
    if dir == 0:
        return (d.joff, d.joff + d.nj), (d.ioff - 1, d.ioff + d.ni), (0, 1)
    return (d.joff - 1, d.joff + d.nj), (d.ioff, d.ioff + d.ni), (1, 0)


def _A(d, a, rng, di=0, dj=0):
    """The part of `a` on local inclusive ranges rng = (i0, i1, j0, j1), shifted by (di, dj)."""
    i0, i1, j0, j1 = rng
    return a[(Ellipsis,) + d.sl(i0 + di, i1 + di, j0 + dj, j1 + dj)]


def _derivs(orc, eos, T, S, p):
    """dR_dT, dR_dS of the oracle's EOS (oracle/orc.py eos_density_derivs), one point at a time."""
    a, b = np.empty(T.shape), np.empty(T.shape)
    fa, fb = a.reshape(-1), b.reshape(-1)
    f = orc.eos_density_derivs
    for n, (t, s, q) in enumerate(zip(T.reshape(-1).tolist(), S.reshape(-1).tolist(), p.reshape(-1).tolist())):
        fa[n], fb[n] = f(eos, t, s, q)
    return a, b


def find_eta(d, M, h, H_to_Z):
    """find_eta, Boussinesq, dZ_ref = 0 (MOM_interface_heights.F90:91-97), on every column of the array."""
    nz = d.nk
    e = np.empty((nz + 1,) + h.shape[1:])
    e[nz] = -(M[G["bathyT"]] + 0.0)
    for k in range(nz - 1, -1, -1):
        e[k] = e[k + 1] + h[k] * H_to_Z
    return e


def pressure_column(h, p_surf, gH):
    """pres at the nz + 1 interfaces, summed top-down with gH = g_Earth * H_to_RZ (MOM_isopycnal_slopes.F90:231-247,
    MOM_thickness_diffuse.F90:864-882)."""
    nz = h.shape[0]
    pres = np.empty((nz + 1,) + h.shape[1:])
    pres[0] = 0.0
    if p_surf is not None:
        pres[0] = p_surf
    for k in range(nz):
        pres[k + 1] = pres[k] + gH * h[k]
    return pres


def vert_fill_TS(h, T_in, S_in, kappa_dt, GV, Z_to_H_fill, larger_h_denom, counts=None):
    """vert_fill_TS on every column of the arrays; `larger_h_denom` as the routine's optional argument (thickness_diffuse_full
    passes .true., calc_isoneutral_slopes leaves it out)."""
    nz = h.shape[0]
    h_neglect = GV.H_subroundoff
    kap_dt_x2 = (2.0 * kappa_dt) * Z_to_H_fill                    # :655
    if kap_dt_x2 <= 0.0:                                          # :661-665
        if counts is not None:
            counts["kap_zero"] += 1
        return T_in.copy(), S_in.copy()
    h0 = 1.0e-16 * np.sqrt(0.5 * kap_dt_x2) if larger_h_denom else h_neglect   # :656-659
    T_f, S_f = np.empty_like(T_in), np.empty_like(S_in)
    c1 = np.zeros_like(h)
    ent = kap_dt_x2 / ((h[0] + h[1]) + h0)                        # :670-675
    h_tr = h[0] + h_neglect
    b1 = 1.0 / (h_tr + ent)
    d1 = b1 * h_tr
    T_f[0] = (b1 * h_tr) * T_in[0]
    S_f[0] = (b1 * h_tr) * S_in[0]
    for k in range(1, nz - 1):                                    # :677-685
        entn = kap_dt_x2 / ((h[k] + h[k + 1]) + h0)
        h_tr = h[k] + h_neglect
        c1[k] = ent * b1
        b1 = 1.0 / ((h_tr + d1 * ent) + entn)
        d1 = b1 * (h_tr + d1 * ent)
        T_f[k] = b1 * (h_tr * T_in[k] + ent * T_f[k - 1])
        S_f[k] = b1 * (h_tr * S_in[k] + ent * S_f[k - 1])
        ent = entn
    c1[nz - 1] = ent * b1                                         # :687-691
    h_tr = h[nz - 1] + h_neglect
    b1 = 1.0 / (h_tr + d1 * ent)
    T_f[nz - 1] = b1 * (h_tr * T_in[nz - 1] + ent * T_f[nz - 2])
    S_f[nz - 1] = b1 * (h_tr * S_in[nz - 1] + ent * S_f[nz - 2])
    for k in range(nz - 2, -1, -1):                               # :693-696
        T_f[k] = T_f[k] + c1[k + 1] * T_f[k + 1]
        S_f[k] = S_f[k] + c1[k + 1] * S_f[k + 1]
    return T_f, S_f
