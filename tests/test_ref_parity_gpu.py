"""mom6x_set_pen_shortwave, mom6x_energetic_PBL and mom6x_Calculate_kappa_shear on the device against what the reference's own
compiled MOM_opacity.F90, MOM_energetic_PBL.F90 and MOM_kappa_shear.F90 gave on the same seeded inputs: the recorded results
tests/golden/ref_opacity_*.npz, ref_epbl_*.npz and ref_kshear_*.npz
(scripts/record_ref_parity.py wrote them from oracle/_ref/libref_param.so; tests/test_ref_parity_cpu.py holds the restatements
and the live library to the same files).  Nothing here needs the compiled reference.

Exactly the recorded cases: manizza_3, morel_1 and ohlmann_1 on a basin with an island at 4 layers; croot_new and rh18_orig_tl (rh18_orig at a transition scale the reference's init accepts) on a
bowl at 3 and 8 layers; each of the five on a land-free torus one cell larger than a work-group in each direction.  Bit for bit on
the computational domain; opac_diag, a tanh, to the project's bound of 1e-12 of its range.  Every output starts as NaN and its halo
must still be NaN.  mstar_sfc and ustar_diag are compared at wet points, where the reference defines them; OBL_its reaches no
diagnostic of the reference and is not recorded.

Kind kshear: shear, bugs, nkml2, layered, newton and tie on the basin with an island at 4 layers, shear and nkml2 on the bowl at 8, shear
on the bowl at 2, shear and layered on the torus at 3.  The device is fed u and v (its own find_uv_at_h runs; the compiled routine
was handed the restatement's u_h, v_h) with NaN halos; kappa_io, tke_io, kv_io and the four 3-D diagnostics bit for bit, there is
no tolerance class; no halo exchange happens.  KS_its reaches no diagnostic of the reference and is not recorded."""
import numpy as np
import pytest

from mom6_amd import abi
from tests import helpers as H
from tests import opacity_ref
from tests import ref_param as RP

pytestmark = pytest.mark.gpu
G = abi.G
BOUND = 1.0e-12


def _ids():
    return [RP.golden_name(*c) for c in RP.golden_configs()]


def _compare(tag, kind, d, M, gold, got):
    dm = RP.dom(d)
    wet = (M[G["mask2dT"]] > 0.0)[dm]
    halo = np.ones(d.shape2(), bool)
    halo[H.interior(d, "h")] = False
    names = set(got) - set(RP.EPBL_NOT_EXPOSED) - set(RP.KSHEAR_NOT_EXPOSED)
    if kind == "kshear":                 # (a file that would pass the size limit leaves out diagnostics)
        assert set(RP.KSHEAR_CORE) <= set(gold) <= names, (sorted(gold), sorted(got))
    else:
        assert set(gold) == names, (sorted(gold), sorted(got))
    for n, a in got.items():
        assert np.isnan(a[..., halo]).all() and np.isfinite(a[..., ~halo]).all(), (tag, n)
    for n, b in gold.items():
        a = np.ascontiguousarray(got[n][(Ellipsis,) + dm])
        if n in RP.EPBL_WET_ONLY:
            a, b = a[..., wet], b[..., wet]
        if n in opacity_ref.OUT_TRANSCENDENTAL:
            rng = float(b.max() - b.min()) or float(np.abs(b).max())
            r = float(np.abs(a - b).max() / rng)
            print(tag, n, "largest difference / range", r)
            assert r <= BOUND, (tag, n, r)
        else:
            H.assert_bitwise(a, np.ascontiguousarray(b), f"{tag}: {n}")


@pytest.mark.parametrize("kind,name,grid,kw", RP.golden_configs(), ids=_ids())
def test_device_against_the_recorded_reference(kind, name, grid, kw):
    d, M, GV, P, opt, inp = RP.golden_setup(kind, name, grid, kw)
    gold = RP.load_golden(kind, name, grid, kw, M, inp)           # (the stored SHA-256 of every input is checked here)
    tag = RP.golden_name(kind, name, grid, kw)
    if kind == "opacity":
        from tests.test_opacity_gpu import _Dy, _device
        with _Dy(d, M, GV) as dy:
            got, neg = _device(dy, d, P, opt, inp)
        assert neg == 0
    elif kind == "kshear":
        from tests.test_kappa_shear_gpu import _device, _nan_halo
        got, nex = _device(d, M, GV, P, opt, _nan_halo(d, inp))
        assert nex == 0
    else:
        from tests.test_energetic_PBL_gpu import _device, _nan_halo
        got, nex = _device(d, M, GV, P, opt, _nan_halo(d, inp))
        assert nex == 0
    _compare(tag, kind, d, M, gold, got)
