!> Start-up check a Fortran host performs: the bind(C) mirrors have the sizes the C library was built with.
program check_abi
  use, intrinsic :: iso_c_binding
  use mom6x_c_api
  implicit none
  type(mom6x_dims) :: d
  type(mom6x_vgrid) :: gv
  type(mom6x_continuity_params) :: cp
  type(mom6x_BT_cont) :: btc
  type(mom6x_barotropic_params) :: bp
  type(mom6x_coriolis_params) :: co
  type(mom6x_pgf_params) :: pg
  type(mom6x_rk2_params) :: rk
  type(mom6x_rk2_hooks) :: hk
  type(mom6x_eos_params) :: eo
  type(mom6x_vertvisc_params) :: vv
  type(mom6x_hor_visc_params) :: hv
  type(mom6x_remapping_params) :: rm
  type(mom6x_regrid_zstar_params) :: rz
  type(mom6x_chksum_result) :: cr
  type(mom6x_sum_output_params) :: sp
  type(mom6x_energy_sums) :: es
  type(mom6x_regrid_rho_params) :: rr
  type(mom6x_set_visc_params) :: sv
  type(mom6x_thickness_diffuse_params) :: td
  type(mom6x_tracer_hor_diff_params) :: thd
  type(mom6x_varmix_params) :: vm
  type(mom6x_mixedlayer_restrat_params) :: mle
  type(mom6x_set_diffusivity_params) :: sd
  type(mom6x_diabatic_aux_params) :: da
  type(mom6x_surface_fluxes) :: sf
  type(mom6x_energetic_PBL_params) :: ep
  type(mom6x_frazil_params) :: fz
  type(mom6x_geothermal_params) :: geo
  type(mom6x_opacity_params) :: opa
  type(mom6x_kappa_shear_params) :: ksp
  type(mom6x_neutral_diffusion_params) :: ndp
  integer :: nbad, rc
  nbad = 0
  call chk(0, int(c_sizeof(d)), "mom6x_dims")
  call chk(1, int(c_sizeof(gv)), "mom6x_vgrid")
  call chk(2, int(c_sizeof(cp)), "mom6x_continuity_params")
  call chk(3, int(c_sizeof(btc)), "mom6x_BT_cont")
  call chk(4, int(c_sizeof(bp)), "mom6x_barotropic_params")
  call chk(5, int(c_sizeof(co)), "mom6x_coriolis_params")
  call chk(6, int(c_sizeof(pg)), "mom6x_pgf_params")
  call chk(7, int(c_sizeof(rk)), "mom6x_rk2_params")
  call chk(8, int(c_sizeof(hk)), "mom6x_rk2_hooks")
  call chk(9, int(c_sizeof(eo)), "mom6x_eos_params")
  call chk(10, int(c_sizeof(vv)), "mom6x_vertvisc_params")
  call chk(11, int(c_sizeof(hv)), "mom6x_hor_visc_params")
  call chk(12, int(c_sizeof(rm)), "mom6x_remapping_params")
  call chk(13, int(c_sizeof(rz)), "mom6x_regrid_zstar_params")
  call chk(14, int(c_sizeof(cr)), "mom6x_chksum_result")
  call chk(15, int(c_sizeof(sp)), "mom6x_sum_output_params")
  call chk(16, int(c_sizeof(es)), "mom6x_energy_sums")
  call chk(17, int(c_sizeof(rr)), "mom6x_regrid_rho_params")
  call chk(18, int(c_sizeof(sv)), "mom6x_set_visc_params")
  call chk(19, int(c_sizeof(td)), "mom6x_thickness_diffuse_params")
  call chk(20, int(c_sizeof(thd)), "mom6x_tracer_hor_diff_params")
  call chk(21, int(c_sizeof(vm)), "mom6x_varmix_params")
  call chk(22, int(c_sizeof(mle)), "mom6x_mixedlayer_restrat_params")
  call chk(25, int(c_sizeof(sd)), "mom6x_set_diffusivity_params")
  call chk(27, int(c_sizeof(da)), "mom6x_diabatic_aux_params")
  call chk(28, int(c_sizeof(sf)), "mom6x_surface_fluxes")
  call chk(30, int(c_sizeof(ep)), "mom6x_energetic_PBL_params")
  call chk(32, int(c_sizeof(fz)), "mom6x_frazil_params")
  call chk(33, int(c_sizeof(geo)), "mom6x_geothermal_params")
  call chk(34, int(c_sizeof(opa)), "mom6x_opacity_params")
  call chk(35, int(c_sizeof(ksp)), "mom6x_kappa_shear_params")
  call chk(36, int(c_sizeof(ndp)), "mom6x_neutral_diffusion_params")
  if (mom6x_abi_version() /= MOM6X_ABI_BUILT_FOR) then
    print '(a,i0,a,i0)', "ABI version: library ", mom6x_abi_version(), ", fortran/mom6x_c_api.F90 ", MOM6X_ABI_BUILT_FOR ; nbad = nbad + 1
  endif
  rc = mom6x_dims_init(d, 1440, 1080, 75, 4)
  if (rc /= 0 .or. d%pitch /= 1472 .or. d%ioff /= 16) then
    print *, "mom6x_dims_init mismatch", rc, d%pitch, d%ioff ; nbad = nbad + 1
  endif
  if (nbad == 0) then
    print '(a)', "fortran ABI check OK"
  else
    print '(a,i0)', "fortran ABI check FAILED: ", nbad
    stop 1
  endif
contains
  subroutine chk(which, fsize, name)
    integer, intent(in) :: which, fsize
    character(len=*), intent(in) :: name
    if (mom6x_struct_size(int(which, c_int)) /= fsize) then
      print *, "size mismatch for ", name, mom6x_struct_size(int(which, c_int)), fsize
      nbad = nbad + 1
    endif
  end subroutine chk
end program check_abi
