!> ORACLE SUPPORT (test infrastructure only): bind(C) doors into the reference's parameterization modules, compiled where
!! they lie against the stand-ins of oracle/ref_standins.F90 into oracle/_ref/libref_param.so (see oracle/Makefile):
!! MOM_EOS_Wright.F90, MOM_EOS_Wright_full.F90, MOM_EOS_Wright_red.F90, MOM_EOS_linear.F90, MOM_intrinsic_functions.F90,
!! MOM_opacity.F90, MOM_energetic_PBL.F90, MOM_kappa_shear.F90, MOM_neutral_diffusion.F90, MOM_isopycnal_slopes.F90,
!! MOM_lateral_mixing_coeffs.F90 and MOM_thickness_diffuse.F90 (with the dispatcher MOM_EOS.F90 that the last five call and the
!! find_eta and thickness_to_dz of MOM_interface_heights.F90), with MOM_unit_scaling.F90 and MOM_string_functions.F90.
!! tests/ref_param.py loads the library and holds the parameter-name maps; tests/test_ref_parity_cpu.py holds the python
!! restatements under tests/ to these doors.  Nothing of the reference is copied here.
!!
!! Arrays come in the project's pitched tile layout: a plane is [nj_mem, ni_mem] in C order, which is (ni_mem, nj_mem) here, so
!! the data domain is isd = jsd = 1, ied = ni_mem, jed = nj_mem, and idx = (isc, iec, jsc, jec) names the computational domain
!! (1-based).  Planes at vorticity points have the same extents (IsdB = 1), the point (I, J) lying north-east of (i, j).
!! vgr = (Rho0, g_Earth_Z_T2, Angstrom_H, Angstrom_Z, H_subroundoff, dZ_subroundoff, H_to_Z, Z_to_H, H_to_RZ, RZ_to_H, H_to_m,
!! m_to_H, H_to_MKS, HZ_T_to_m2_s).  Every door that runs a module returns the number of FATAL messages it met.
module ref_param_shim
  use, intrinsic :: iso_c_binding
  use MOM_error_handler, only : standin_fatal_count, standin_never_count
  use MOM_file_parser, only : param_file_type, standin_clear_params, standin_set_real, standin_set_int, standin_set_char, &
                              standin_set_reals
  use MOM_diag_mediator, only : diag_ctrl, time_type, standin_clear_diags, standin_want_diag, standin_diag_size, standin_get_diag
  use MOM_diag_mediator, only : axes_grp, register_diag_field
  use MOM_grid, only : ocean_grid_type
  use MOM_verticalGrid, only : verticalGrid_type
  use MOM_unit_scaling, only : unit_scale_type, unit_scaling_init, unit_scaling_end
  use MOM_variables, only : thermo_var_ptrs, vertvisc_type
  use MOM_EOS, only : EOS_type, EOS_init
  use MOM_forcing_type, only : forcing
  use MOM_wave_interface, only : wave_parameters_CS
  use MOM_stochastics, only : stochastic_CS
  use MOM_EOS_Wright, only : buggy_Wright_EOS
  use MOM_EOS_Wright_full, only : Wright_full_EOS
  use MOM_EOS_Wright_red, only : Wright_red_EOS
  use MOM_EOS_linear, only : linear_EOS
  use MOM_EOS_base_type, only : EOS_base
  use MOM_intrinsic_functions, only : cuberoot, invcosh
  use MOM_opacity, only : optics_type, opacity_CS, opacity_init, set_opacity, opacity_end, absorbRemainingSW, sumSWoverBands
  use MOM_energetic_PBL, only : energetic_PBL_CS, energetic_PBL_init, energetic_PBL, energetic_PBL_get_MLD, energetic_PBL_end
  use MOM_kappa_shear, only : Kappa_shear_CS, kappa_shear_init, Calculate_kappa_shear
  use MOM_neutral_diffusion, only : neutral_diffusion_CS, neutral_diffusion_init, neutral_diffusion_calc_coeffs, neutral_diffusion, &
                                    neutral_diffusion_end
  use MOM_tracer_registry, only : tracer_registry_type
  use MOM_variables, only : cont_diag_ptrs
  use MOM_open_boundary, only : ocean_OBC_type
  use MOM_MEKE_types, only : MEKE_type
  use MOM_lateral_mixing_coeffs, only : VarMix_CS, VarMix_init, VarMix_end, calc_slope_functions
  use MOM_thickness_diffuse, only : thickness_diffuse_CS, thickness_diffuse_init, thickness_diffuse, thickness_diffuse_end
  use MOM_diabatic_driver, only : diabatic_CS
  implicit none
contains
  function fstr(s) result(f)
    character(kind=c_char), intent(in) :: s(*) ; character(len=:), allocatable :: f ; integer :: n, m
    n = 0
    do while (s(n+1) /= c_null_char) ; n = n + 1 ; enddo
    allocate(character(len=n) :: f)
    do m = 1, n ; f(m:m) = s(m) ; enddo
  end function fstr

  ! ---- the parameter table, the diagnostics asked for and the capture store ----
  subroutine ref_param_clear() bind(C, name="ref_param_clear")
    call standin_clear_params() ; call standin_clear_diags() ; standin_fatal_count = 0 ; standin_never_count = 0
  end subroutine
  subroutine ref_set_real(name, value) bind(C, name="ref_set_real")
    character(kind=c_char), intent(in) :: name(*) ; real(c_double), value :: value
    call standin_set_real(fstr(name), value)
  end subroutine
  subroutine ref_set_reals(name, n, values) bind(C, name="ref_set_reals")
    character(kind=c_char), intent(in) :: name(*) ; integer(c_int), value :: n ; real(c_double), intent(in) :: values(n)
    call standin_set_reals(fstr(name), values)
  end subroutine
  subroutine ref_set_int(name, value) bind(C, name="ref_set_int")
    character(kind=c_char), intent(in) :: name(*) ; integer(c_int), value :: value
    call standin_set_int(fstr(name), int(value))
  end subroutine
  subroutine ref_set_char(name, value) bind(C, name="ref_set_char")
    character(kind=c_char), intent(in) :: name(*), value(*)
    call standin_set_char(fstr(name), fstr(value))
  end subroutine
  subroutine ref_want_diag(name) bind(C, name="ref_want_diag")
    character(kind=c_char), intent(in) :: name(*)
    call standin_want_diag(fstr(name))
  end subroutine
  integer(c_int) function ref_diag_size(name) bind(C, name="ref_diag_size")
    character(kind=c_char), intent(in) :: name(*)
    ref_diag_size = standin_diag_size(fstr(name))
  end function
  subroutine ref_get_diag(name, n, out) bind(C, name="ref_get_diag")
    character(kind=c_char), intent(in) :: name(*) ; integer(c_int), value :: n ; real(c_double), intent(inout) :: out(n)
    call standin_get_diag(fstr(name), out)
  end subroutine

  ! ---- equations of state and intrinsic functions ----
  subroutine eos_points(eos, n, T, S, p, rho_ref, rho, rho_anom, spv, drho_dT, drho_dS, dSV_dT, dSV_dS, rho_c, drho_dp)
    class(EOS_base), intent(in) :: eos ; integer, intent(in) :: n
    real, intent(in) :: T(n), S(n), p(n), rho_ref
    real, intent(out) :: rho(n), rho_anom(n), spv(n), drho_dT(n), drho_dS(n), dSV_dT(n), dSV_dS(n), rho_c(n), drho_dp(n)
    integer :: i
    do i = 1, n
      rho(i) = eos%density_elem(T(i), S(i), p(i))
      rho_anom(i) = eos%density_anomaly_elem(T(i), S(i), p(i), rho_ref)
      spv(i) = eos%spec_vol_elem(T(i), S(i), p(i))
      call eos%calculate_density_derivs_elem(T(i), S(i), p(i), drho_dT(i), drho_dS(i))
      call eos%calculate_specvol_derivs_elem(T(i), S(i), p(i), dSV_dT(i), dSV_dS(i))
      call eos%calculate_compress_elem(T(i), S(i), p(i), rho_c(i), drho_dp(i))
    enddo
  end subroutine eos_points
  !> src/equation_of_state/MOM_EOS_Wright.F90 (the default WRIGHT): density_elem, density_anomaly_elem, spec_vol_elem,
  !! calculate_density_derivs_elem, calculate_specvol_derivs_elem and calculate_compress_elem of n points.
  subroutine ref_WRIGHT(n, T, S, p, rho_ref, rho, rho_anom, spv, drho_dT, drho_dS, dSV_dT, dSV_dS, rho_c, drho_dp) &
      bind(C, name="ref_WRIGHT")
    integer(c_int), value :: n ; real(c_double), intent(in) :: T(n), S(n), p(n) ; real(c_double), value :: rho_ref
    real(c_double), intent(out) :: rho(n), rho_anom(n), spv(n), drho_dT(n), drho_dS(n), dSV_dT(n), dSV_dS(n), rho_c(n), drho_dp(n)
    type(buggy_Wright_EOS) :: eos
    call eos_points(eos, int(n), T, S, p, rho_ref, rho, rho_anom, spv, drho_dT, drho_dS, dSV_dT, dSV_dS, rho_c, drho_dp)
  end subroutine
  !> src/equation_of_state/MOM_EOS_Wright_full.F90 likewise.
  subroutine ref_WRIGHT_FULL(n, T, S, p, rho_ref, rho, rho_anom, spv, drho_dT, drho_dS, dSV_dT, dSV_dS, rho_c, drho_dp) &
      bind(C, name="ref_WRIGHT_FULL")
    integer(c_int), value :: n ; real(c_double), intent(in) :: T(n), S(n), p(n) ; real(c_double), value :: rho_ref
    real(c_double), intent(out) :: rho(n), rho_anom(n), spv(n), drho_dT(n), drho_dS(n), dSV_dT(n), dSV_dS(n), rho_c(n), drho_dp(n)
    type(Wright_full_EOS) :: eos
    call eos_points(eos, int(n), T, S, p, rho_ref, rho, rho_anom, spv, drho_dT, drho_dS, dSV_dT, dSV_dS, rho_c, drho_dp)
  end subroutine
  !> src/equation_of_state/MOM_EOS_Wright_red.F90 likewise.
  subroutine ref_WRIGHT_REDUCED(n, T, S, p, rho_ref, rho, rho_anom, spv, drho_dT, drho_dS, dSV_dT, dSV_dS, rho_c, drho_dp) &
      bind(C, name="ref_WRIGHT_REDUCED")
    integer(c_int), value :: n ; real(c_double), intent(in) :: T(n), S(n), p(n) ; real(c_double), value :: rho_ref
    real(c_double), intent(out) :: rho(n), rho_anom(n), spv(n), drho_dT(n), drho_dS(n), dSV_dT(n), dSV_dS(n), rho_c(n), drho_dp(n)
    type(Wright_red_EOS) :: eos
    call eos_points(eos, int(n), T, S, p, rho_ref, rho, rho_anom, spv, drho_dT, drho_dS, dSV_dT, dSV_dS, rho_c, drho_dp)
  end subroutine
  !> src/equation_of_state/MOM_EOS_linear.F90 likewise, the coefficients set through set_params_linear (:255).
  subroutine ref_LINEAR(n, T, S, p, rho_ref, coef, rho, rho_anom, spv, drho_dT, drho_dS, dSV_dT, dSV_dS, rho_c, drho_dp) &
      bind(C, name="ref_LINEAR")
    integer(c_int), value :: n ; real(c_double), intent(in) :: T(n), S(n), p(n), coef(4) ; real(c_double), value :: rho_ref
    real(c_double), intent(out) :: rho(n), rho_anom(n), spv(n), drho_dT(n), drho_dS(n), dSV_dT(n), dSV_dS(n), rho_c(n), drho_dp(n)
    type(linear_EOS) :: eos
    call eos%set_params_linear(Rho_T0_S0=coef(1), dRho_dT=coef(2), dRho_dS=coef(3), dRho_dp=coef(4))
    call eos_points(eos, int(n), T, S, p, rho_ref, rho, rho_anom, spv, drho_dT, drho_dS, dSV_dT, dSV_dS, rho_c, drho_dp)
  end subroutine
  !> src/framework/MOM_intrinsic_functions.F90: cuberoot :48 and invcosh :32.
  subroutine ref_cuberoot(n, x, y) bind(C, name="ref_cuberoot")
    integer(c_int), value :: n ; real(c_double), intent(in) :: x(n) ; real(c_double), intent(out) :: y(n) ; integer :: i
    do i = 1, n ; y(i) = cuberoot(x(i)) ; enddo
  end subroutine
  subroutine ref_invcosh(n, x, y) bind(C, name="ref_invcosh")
    integer(c_int), value :: n ; real(c_double), intent(in) :: x(n) ; real(c_double), intent(out) :: y(n) ; integer :: i
    do i = 1, n ; y(i) = invcosh(x(i)) ; enddo
  end subroutine

  ! ---- the grid, the vertical grid and the unit scaling of a door ----
  subroutine setup(ni_mem, nj_mem, idx, nk, vgr, mask, cor, pf, G, GV, US)
    integer, intent(in) :: ni_mem, nj_mem, idx(4), nk ; real, intent(in) :: vgr(14), mask(ni_mem, nj_mem)
    type(c_ptr), intent(in) :: cor ; type(param_file_type), intent(in) :: pf
    type(ocean_grid_type), intent(inout) :: G ; type(verticalGrid_type), intent(inout) :: GV ; type(unit_scale_type), pointer :: US
    real, pointer :: f(:,:)
    G%isd = 1 ; G%ied = ni_mem ; G%jsd = 1 ; G%jed = nj_mem ; G%IsdB = 1 ; G%IedB = ni_mem ; G%JsdB = 1 ; G%JedB = nj_mem
    G%isc = idx(1) ; G%iec = idx(2) ; G%jsc = idx(3) ; G%jec = idx(4)
    G%IscB = G%isc - 1 ; G%IecB = G%iec ; G%JscB = G%jsc - 1 ; G%JecB = G%jec
    G%HI%isd = G%isd ; G%HI%ied = G%ied ; G%HI%jsd = G%jsd ; G%HI%jed = G%jed ; G%HI%isc = G%isc ; G%HI%iec = G%iec
    G%HI%jsc = G%jsc ; G%HI%jec = G%jec ; G%HI%IsdB = G%IsdB ; G%HI%IedB = G%IedB ; G%HI%JsdB = G%JsdB ; G%HI%JedB = G%JedB
    G%HI%IscB = G%IscB ; G%HI%IecB = G%IecB ; G%HI%JscB = G%JscB ; G%HI%JecB = G%JecB
    allocate(G%mask2dT(ni_mem, nj_mem), G%CoriolisBu(ni_mem, nj_mem), G%geoLonT(ni_mem, nj_mem), G%geoLatT(ni_mem, nj_mem))
    G%mask2dT(:,:) = mask(:,:) ; G%CoriolisBu(:,:) = 0.0 ; G%geoLonT(:,:) = 0.0 ; G%geoLatT(:,:) = 0.0
    if (c_associated(cor)) then
      call c_f_pointer(cor, f, (/ ni_mem, nj_mem /)) ; G%CoriolisBu(:,:) = f(:,:)
    endif
    GV%ke = nk ; GV%Boussinesq = .true.
    GV%Rho0 = vgr(1) ; GV%g_Earth_Z_T2 = vgr(2) ; GV%Angstrom_H = vgr(3) ; GV%Angstrom_Z = vgr(4) ; GV%H_subroundoff = vgr(5)
    GV%dZ_subroundoff = vgr(6) ; GV%H_to_Z = vgr(7) ; GV%Z_to_H = vgr(8) ; GV%H_to_RZ = vgr(9) ; GV%RZ_to_H = vgr(10)
    GV%H_to_m = vgr(11) ; GV%m_to_H = vgr(12) ; GV%H_to_MKS = vgr(13) ; GV%HZ_T_to_m2_s = vgr(14)
    US => NULL()
    call unit_scaling_init(pf, US)   ! the reference's own, from the *_RESCALE_POWER entries of the table
  end subroutine setup
  subroutine plane(p, ni_mem, nj_mem, f)
    type(c_ptr), intent(in) :: p ; integer, intent(in) :: ni_mem, nj_mem ; real, pointer :: f(:,:)
    f => NULL()
    if (c_associated(p)) call c_f_pointer(p, f, (/ ni_mem, nj_mem /))
  end subroutine plane

  !> opacity_init (MOM_opacity.F90:1019) through the table, then set_opacity (:118) on whole arrays.  The shortwave planes and the
  !! chlorophyll arrays are C pointers, null for "not associated" / "not present".  opacity_band [nbands, nk, nj_mem, ni_mem] and
  !! sw_pen_band [nbands, nj_mem, ni_mem] get optics%opacity_band and optics%sw_pen_band; nbands_out gets optics%nbands.  The
  !! diagnostics asked for with ref_want_diag (SW_pen, SW_vis_pen, opac_1 ...) are read back with ref_get_diag.
  integer(c_int) function ref_opacity(ni_mem, nj_mem, idx, nk, vgr, mask, sw, vis_dir, vis_dif, nir_dir, nir_dif, chl_2d, chl_3d, &
                                      nb_max, nbands_out, opacity_band, sw_pen_band) bind(C, name="ref_opacity")
    integer(c_int), value :: ni_mem, nj_mem, nk, nb_max ; integer(c_int), intent(in) :: idx(4)
    real(c_double), intent(in) :: vgr(14), mask(ni_mem, nj_mem)
    type(c_ptr), value :: sw, vis_dir, vis_dif, nir_dir, nir_dif, chl_2d, chl_3d
    integer(c_int), intent(out) :: nbands_out
    real(c_double), intent(inout) :: opacity_band(ni_mem, nj_mem, nk, nb_max), sw_pen_band(ni_mem, nj_mem, nb_max)
    type(ocean_grid_type) :: G ; type(verticalGrid_type) :: GV ; type(unit_scale_type), pointer :: US
    type(param_file_type) :: pf ; type(diag_ctrl), target :: diag ; type(time_type), target :: Time
    type(opacity_CS) :: CS ; type(optics_type) :: optics
    real, pointer, dimension(:,:) :: p_sw, p_vd, p_vf, p_nd, p_nf, c2
    real, pointer :: c3(:,:,:)
    integer :: i, j, k, n
    standin_fatal_count = 0
    call setup(int(ni_mem), int(nj_mem), int(idx), int(nk), vgr, mask, c_null_ptr, pf, G, GV, US)
    call opacity_init(Time, G, GV, US, pf, diag, CS, optics)
    nbands_out = optics%nbands
    if (standin_fatal_count == 0 .and. optics%nbands <= nb_max) then
      call plane(sw, int(ni_mem), int(nj_mem), p_sw) ; call plane(vis_dir, int(ni_mem), int(nj_mem), p_vd)
      call plane(vis_dif, int(ni_mem), int(nj_mem), p_vf) ; call plane(nir_dir, int(ni_mem), int(nj_mem), p_nd)
      call plane(nir_dif, int(ni_mem), int(nj_mem), p_nf) ; call plane(chl_2d, int(ni_mem), int(nj_mem), c2)
      c3 => NULL() ; if (c_associated(chl_3d)) call c_f_pointer(chl_3d, c3, (/ int(ni_mem), int(nj_mem), int(nk) /))
      if (associated(c2)) then
        call set_opacity(optics, p_sw, p_vd, p_vf, p_nd, p_nf, G, GV, US, CS, chl_2d=c2)
      elseif (associated(c3)) then
        call set_opacity(optics, p_sw, p_vd, p_vf, p_nd, p_nf, G, GV, US, CS, chl_3d=c3)
      else
        call set_opacity(optics, p_sw, p_vd, p_vf, p_nd, p_nf, G, GV, US, CS)
      endif
      do n = 1, optics%nbands
        do k = 1, nk ; do j = 1, nj_mem ; do i = 1, ni_mem
          opacity_band(i,j,k,n) = optics%opacity_band(n,i,j,k)
        enddo ; enddo ; enddo
        do j = G%jsc, G%jec ; do i = G%isc, G%iec
          sw_pen_band(i,j,n) = optics%sw_pen_band(n,i,j)
        enddo ; enddo
      enddo
    endif
    call opacity_end(CS, optics)
    call unit_scaling_end(US)
    ref_opacity = standin_fatal_count
  end function

  !> absorbRemainingSW (MOM_opacity.F90:600) on one j-row of ni points and nk layers, with the optional TKE and dSV_dT (C
  !! pointers, null: absent).  optics carries nbands, answer_date, PenSW_flux_absorb and PenSW_absorb_Invlen, which is all that
  !! the routine reads of it.  h, T, TKE, dSV_dT are [nk, ni]; opacity_band [nk, ni, nsw_mem] and Pen_SW_bnd [ni, nsw_mem] with
  !! nsw_mem = max(nsw, 1), the band first as in the reference.
  integer(c_int) function ref_absorbRemainingSW(ni, nk, vgr, nsw, answer_date, PenSW_flux_absorb, PenSW_absorb_Invlen, h, &
        opacity_band, dt, H_limit_fluxes, adjustAbsorptionProfile, absorbAllSW, T, Pen_SW_bnd, TKE, dSV_dT) &
        bind(C, name="ref_absorbRemainingSW")
    integer(c_int), value :: ni, nk, nsw, answer_date, adjustAbsorptionProfile, absorbAllSW
    real(c_double), intent(in) :: vgr(14), h(ni, nk), opacity_band(max(1,nsw), ni, nk)
    real(c_double), value :: PenSW_flux_absorb, PenSW_absorb_Invlen, dt, H_limit_fluxes
    real(c_double), intent(inout) :: T(ni, nk), Pen_SW_bnd(max(1,nsw), ni)
    type(c_ptr), value :: TKE, dSV_dT
    type(ocean_grid_type) :: G ; type(verticalGrid_type) :: GV ; type(unit_scale_type), pointer :: US
    type(param_file_type) :: pf ; type(optics_type) :: optics
    real :: mask(ni, 1)
    real, pointer :: p_TKE(:,:), p_dSV(:,:)
    standin_fatal_count = 0
    mask(:,:) = 1.0
    call setup(int(ni), 1, (/ 1, int(ni), 1, 1 /), int(nk), vgr, mask, c_null_ptr, pf, G, GV, US)
    optics%nbands = nsw ; optics%answer_date = answer_date
    optics%PenSW_flux_absorb = PenSW_flux_absorb ; optics%PenSW_absorb_Invlen = PenSW_absorb_Invlen
    if (c_associated(TKE) .and. c_associated(dSV_dT)) then
      call c_f_pointer(TKE, p_TKE, (/ int(ni), int(nk) /)) ; call c_f_pointer(dSV_dT, p_dSV, (/ int(ni), int(nk) /))
      call absorbRemainingSW(G, GV, US, h, opacity_band, int(nsw), optics, 1, dt, H_limit_fluxes, &
                             (adjustAbsorptionProfile /= 0), (absorbAllSW /= 0), T, Pen_SW_bnd, TKE=p_TKE, dSV_dT=p_dSV)
    else
      call absorbRemainingSW(G, GV, US, h, opacity_band, int(nsw), optics, 1, dt, H_limit_fluxes, &
                             (adjustAbsorptionProfile /= 0), (absorbAllSW /= 0), T, Pen_SW_bnd)
    endif
    call unit_scaling_end(US)
    ref_absorbRemainingSW = standin_fatal_count
  end function

  !> sumSWoverBands (MOM_opacity.F90:873) on one j-row: h, dz [nk, ni]; opacity_band [nk, ni, nsw_mem] goes into
  !! optics%opacity_band of the row; iPen_SW_bnd [ni, nsw_mem]; netPen [nk + 1, ni].
  integer(c_int) function ref_sumSWoverBands(ni, nk, vgr, nsw, answer_date, PenSW_flux_absorb, PenSW_absorb_Invlen, h, dz, &
        opacity_band, dt, H_limit_fluxes, absorbAllSW, iPen_SW_bnd, netPen) bind(C, name="ref_sumSWoverBands")
    integer(c_int), value :: ni, nk, nsw, answer_date, absorbAllSW
    real(c_double), intent(in) :: vgr(14), h(ni, nk), dz(ni, nk), opacity_band(max(1,nsw), ni, nk), iPen_SW_bnd(max(1,nsw), ni)
    real(c_double), value :: PenSW_flux_absorb, PenSW_absorb_Invlen, dt, H_limit_fluxes
    real(c_double), intent(inout) :: netPen(ni, nk+1)
    type(ocean_grid_type) :: G ; type(verticalGrid_type) :: GV ; type(unit_scale_type), pointer :: US
    type(param_file_type) :: pf ; type(optics_type) :: optics
    real :: mask(ni, 1)
    integer :: i, k, n
    standin_fatal_count = 0
    mask(:,:) = 1.0
    call setup(int(ni), 1, (/ 1, int(ni), 1, 1 /), int(nk), vgr, mask, c_null_ptr, pf, G, GV, US)
    optics%nbands = nsw ; optics%answer_date = answer_date
    optics%PenSW_flux_absorb = PenSW_flux_absorb ; optics%PenSW_absorb_Invlen = PenSW_absorb_Invlen
    allocate(optics%opacity_band(max(1,nsw), ni, 1, nk))
    do k = 1, nk ; do i = 1, ni ; do n = 1, max(1,nsw) ; optics%opacity_band(n,i,1,k) = opacity_band(n,i,k) ; enddo ; enddo ; enddo
    call sumSWoverBands(G, GV, US, h, dz, int(nsw), optics, 1, dt, H_limit_fluxes, (absorbAllSW /= 0), iPen_SW_bnd, netPen)
    call unit_scaling_end(US)
    ref_sumSWoverBands = standin_fatal_count
  end function

  !> energetic_PBL_init (MOM_energetic_PBL.F90:3729) through the table, then energetic_PBL (:326) ncalls times on the same
  !! control structure, then energetic_PBL_get_MLD (:3707).  3-D arrays are [nk, nj_mem, ni_mem] (Kd_int: nk + 1 interfaces).
  !! u_h and v_h are the velocities at thickness points (read only with MKE_TO_TKE_EFFIC > 0).  Waves is null and stoch_CS has
  !! pert_epbl false; fluxes carries ustar and ustar_gustless (both the given plane); visc is empty, since every bottom-boundary
  !! option is off.  The diagnostics asked for with ref_want_diag are read back with ref_get_diag.
  integer(c_int) function ref_energetic_PBL(ni_mem, nj_mem, idx, nk, vgr, mask, CoriolisBu, h, u_h, v_h, T, S, dSV_dT, dSV_dS, &
        TKE_forced, ustar, buoy_flux, dt, ncalls, Kd_int, MLD) bind(C, name="ref_energetic_PBL")
    integer(c_int), value :: ni_mem, nj_mem, nk, ncalls ; integer(c_int), intent(in) :: idx(4)
    real(c_double), intent(in) :: vgr(14), mask(ni_mem, nj_mem) ; type(c_ptr), value :: CoriolisBu
    real(c_double), intent(inout) :: h(ni_mem, nj_mem, nk)
    real(c_double), intent(in), dimension(ni_mem, nj_mem, nk) :: u_h, v_h, dSV_dT, dSV_dS, TKE_forced
    real(c_double), intent(inout), target :: T(ni_mem, nj_mem, nk), S(ni_mem, nj_mem, nk), ustar(ni_mem, nj_mem)
    real(c_double), intent(in) :: buoy_flux(ni_mem, nj_mem) ; real(c_double), value :: dt
    real(c_double), intent(inout) :: Kd_int(ni_mem, nj_mem, nk+1), MLD(ni_mem, nj_mem)
    type(ocean_grid_type) :: G ; type(verticalGrid_type) :: GV ; type(unit_scale_type), pointer :: US
    type(param_file_type) :: pf ; type(diag_ctrl), target :: diag ; type(time_type), target :: Time
    type(energetic_PBL_CS) :: CS ; type(thermo_var_ptrs) :: tv ; type(forcing) :: fluxes ; type(vertvisc_type) :: visc
    type(EOS_type), target :: eqn ; type(wave_parameters_CS), pointer :: Waves ; type(stochastic_CS), pointer :: stoch
    real :: BBL_buoy_flux(ni_mem, nj_mem)
    integer :: m
    standin_fatal_count = 0
    call setup(int(ni_mem), int(nj_mem), int(idx), int(nk), vgr, mask, CoriolisBu, pf, G, GV, US)
    call energetic_PBL_init(Time, G, GV, US, pf, diag, CS)
    tv%T => T ; tv%S => S ; tv%eqn_of_state => eqn
    fluxes%ustar => ustar ; fluxes%ustar_gustless => ustar
    Waves => NULL() ; allocate(stoch) ; stoch%pert_epbl = .false.
    BBL_buoy_flux(:,:) = 0.0
    if (standin_fatal_count == 0) then
      do m = 1, ncalls
        call energetic_PBL(h, u_h, v_h, tv, fluxes, visc, dt, Kd_int, G, GV, US, CS, stoch, dSV_dT, dSV_dS, TKE_forced, &
                           buoy_flux, BBL_buoy_flux, Waves)
      enddo
      call energetic_PBL_get_MLD(CS, MLD, G, US)
    endif
    call energetic_PBL_end(CS)
    deallocate(stoch)
    call unit_scaling_end(US)
    ref_energetic_PBL = standin_fatal_count
  end function
  !> kappa_shear_init (MOM_kappa_shear.F90:2070) and EOS_init (MOM_EOS.F90:1540) through the table, then Calculate_kappa_shear
  !! (:133) on a whole tile.  3-D arrays are [nk, nj_mem, ni_mem], the outputs [nk + 1, nj_mem, ni_mem].  u_h and v_h are the
  !! velocities at thickness points (find_uv_at_h lives in MOM_diabatic_aux.F90, which is not compiled).  T and S are C pointers,
  !! null together for the layered arm (tv%T not associated), which reads GV%Rlay = Rlay(nk); p_surf is a C pointer, null for "not
  !! associated".  vgx = (g_Earth, m2_s_to_HZ_T, HZ_T_to_m2_s, HZ_T_to_MKS) are the members of GV beyond vgr that the module reads;
  !! nkml goes in as GV%nkml (read with KAPPA_SHEAR_MERGE_ML).  The diagnostics N2_shear_in, S2_shear_in, N2_shear_mean and
  !! S2_shear_mean are asked for here and read back with ref_get_diag.  dt <= 0: the two inits only (for what they refuse).
  integer(c_int) function ref_Calculate_kappa_shear(ni_mem, nj_mem, idx, nk, vgr, vgx, nkml, mask, Coriolis2Bu, Rlay, h, u_h, v_h, &
        T, S, p_surf, dt, kappa_io, tke_io, kv_io) bind(C, name="ref_Calculate_kappa_shear")
    integer(c_int), value :: ni_mem, nj_mem, nk, nkml ; integer(c_int), intent(in) :: idx(4)
    real(c_double), intent(in) :: vgr(14), vgx(4), mask(ni_mem, nj_mem), Coriolis2Bu(ni_mem, nj_mem), Rlay(nk)
    real(c_double), intent(in), dimension(ni_mem, nj_mem, nk) :: h, u_h, v_h
    type(c_ptr), value :: T, S, p_surf ; real(c_double), value :: dt
    real(c_double), intent(inout), dimension(ni_mem, nj_mem, nk+1) :: kappa_io, tke_io, kv_io
    type(ocean_grid_type) :: G ; type(verticalGrid_type) :: GV ; type(unit_scale_type), pointer :: US
    type(param_file_type) :: pf ; type(diag_ctrl), target :: diag ; type(time_type), target :: Time
    type(Kappa_shear_CS), pointer :: CS ; type(thermo_var_ptrs) :: tv ; type(EOS_type), target :: eqn
    real, pointer :: p_ps(:,:)
    logical :: used
    standin_fatal_count = 0
    call standin_want_diag("N2_shear_in") ; call standin_want_diag("S2_shear_in")
    call standin_want_diag("N2_shear_mean") ; call standin_want_diag("S2_shear_mean")
    call setup(int(ni_mem), int(nj_mem), int(idx), int(nk), vgr, mask, c_null_ptr, pf, G, GV, US)
    allocate(G%Coriolis2Bu(ni_mem, nj_mem), G%mask2dCu(ni_mem, nj_mem), G%mask2dCv(ni_mem, nj_mem), G%mask2dBu(ni_mem, nj_mem))
    G%Coriolis2Bu(:,:) = Coriolis2Bu(:,:) ; G%mask2dCu(:,:) = 0.0 ; G%mask2dCv(:,:) = 0.0 ; G%mask2dBu(:,:) = 0.0  ! (vertex only)
    GV%g_Earth = vgx(1) ; GV%m2_s_to_HZ_T = vgx(2) ; GV%HZ_T_to_m2_s = vgx(3) ; GV%HZ_T_to_MKS = vgx(4)
    GV%nkml = nkml ; GV%semi_Boussinesq = .false.
    allocate(GV%Rlay(nk)) ; GV%Rlay(:) = Rlay(:)
    CS => NULL()
    used = kappa_shear_init(Time, G, GV, US, pf, diag, CS)
    if (.not.used) standin_fatal_count = standin_fatal_count + 1    ! USE_JACKSON_PARAM is part of every table
    if (c_associated(T) .and. c_associated(S)) then
      call c_f_pointer(T, tv%T, (/ int(ni_mem), int(nj_mem), int(nk) /))
      call c_f_pointer(S, tv%S, (/ int(ni_mem), int(nj_mem), int(nk) /))
      call EOS_init(pf, eqn, US)
      tv%eqn_of_state => eqn
    endif
    call plane(p_surf, int(ni_mem), int(nj_mem), p_ps)
    if (standin_fatal_count == 0 .and. dt > 0.0) &
      call Calculate_kappa_shear(u_h, v_h, h, tv, p_ps, kappa_io, tke_io, kv_io, dt, G, GV, US, CS)
    if (associated(CS)) deallocate(CS)
    call unit_scaling_end(US)
    ref_Calculate_kappa_shear = standin_fatal_count
  end function

  !> Of the FATAL messages of the last door, those raised by a stand-in procedure that must never run (a path that leaves the
  !! compiled files: NDIFF_CONTINUOUS false into MOM_remapping, NDIFF_INTERIOR_ONLY into MOM_diabatic_driver).
  integer(c_int) function ref_standin_never_count() bind(C, name="ref_standin_never_count")
    ref_standin_never_count = standin_never_count
  end function

  !> neutral_diffusion_init (MOM_neutral_diffusion.F90:138) and EOS_init through the table, then, `ncalls` times on the same control
  !! structure, neutral_diffusion_calc_coeffs (:351) and neutral_diffusion (:619) over a registry of ntr tracers, on a whole tile.
  !! h, T and S are [ncalls, nk, nj_mem, ni_mem] and p_surf (a C pointer, null: the argument is absent) [ncalls, nj_mem, ni_mem]:
  !! round r computes its coefficients from slice r, so that an array left over from the round before would show.  Coef_x1 and
  !! Coef_y1 are plane 1 of Coef_x and Coef_y; the other nk planes handed to the reference hold NaN.  tracers [ntr, nk, nj_mem,
  !! ni_mem] are changed in place, every round going on from the one before.  masks = (mask2dT, mask2dCu, mask2dCv, IareaT); vgx =
  !! (g_Earth, H_to_pa).  Tracer m's id_dfxy_cont, id_dfx_2d and id_dfy_2d are the ids of the names dfxy_cont_m, dfx_2d_m and
  !! dfy_2d_m (m = 1 ..) where ref_want_diag has asked for them, else -1; id_dfxy_conc and id_dfxy_cont_2d stay -1.  What
  !! post_data last copied (the last round's) is read back with ref_get_diag.  dt <= 0: the two inits only (for what they refuse).
  !! The components of neutral_diffusion_CS are private and id_uhEff_2d, id_vhEff_2d are never registered by the reference:
  !! PoL, PoR, KoL, KoR and hEff cannot be handed out.
  integer(c_int) function ref_neutral_diffusion(ni_mem, nj_mem, idx, nk, vgr, vgx, masks, ncalls, h, T, S, p_surf, Coef_x1, Coef_y1, &
        dt, ntr, tracers, conc_underflow) bind(C, name="ref_neutral_diffusion")
    use, intrinsic :: ieee_arithmetic, only : ieee_value, ieee_quiet_nan
    integer(c_int), value :: ni_mem, nj_mem, nk, ncalls, ntr ; integer(c_int), intent(in) :: idx(4)
    real(c_double), intent(in) :: vgr(14), vgx(2), masks(ni_mem, nj_mem, 4)
    real(c_double), intent(in), target, dimension(ni_mem, nj_mem, nk, ncalls) :: h, T, S
    type(c_ptr), value :: p_surf
    real(c_double), intent(in) :: Coef_x1(ni_mem, nj_mem), Coef_y1(ni_mem, nj_mem), conc_underflow(ntr) ; real(c_double), value :: dt
    real(c_double), intent(inout), target :: tracers(ni_mem, nj_mem, nk, ntr)
    type(ocean_grid_type) :: G ; type(verticalGrid_type) :: GV ; type(unit_scale_type), pointer :: US
    type(param_file_type) :: pf ; type(diag_ctrl), target :: diag ; type(time_type), target :: Time
    type(neutral_diffusion_CS), pointer :: CS ; type(EOS_type), target :: eqn ; type(vertvisc_type) :: visc
    type(diabatic_CS), pointer :: diabatic_CSp ; type(tracer_registry_type), pointer :: Reg ; type(axes_grp) :: axes
    real, allocatable :: Coef_x(:,:,:), Coef_y(:,:,:)
    real, pointer :: p_ps(:,:,:)
    character(len=16) :: tag
    logical :: used
    integer :: m, r
    standin_fatal_count = 0 ; standin_never_count = 0
    call setup(int(ni_mem), int(nj_mem), int(idx), int(nk), vgr, masks(:,:,1), c_null_ptr, pf, G, GV, US)
    allocate(G%mask2dCu(ni_mem, nj_mem), G%mask2dCv(ni_mem, nj_mem), G%IareaT(ni_mem, nj_mem), G%Domain)
    G%mask2dCu(:,:) = masks(:,:,2) ; G%mask2dCv(:,:) = masks(:,:,3) ; G%IareaT(:,:) = masks(:,:,4) ; G%ke = nk
    GV%g_Earth = vgx(1) ; GV%H_to_pa = vgx(2) ; GV%semi_Boussinesq = .false.
    call EOS_init(pf, eqn, US)
    allocate(diabatic_CSp) ; CS => NULL()
    used = neutral_diffusion_init(Time, G, GV, US, pf, diag, eqn, diabatic_CSp, CS)
    if (.not.used) standin_fatal_count = standin_fatal_count + 1      ! USE_NEUTRAL_DIFFUSION is part of every table
    if (standin_fatal_count == 0 .and. dt > 0.0) then
      allocate(Reg) ; allocate(Reg%Tr(ntr)) ; Reg%ntr = ntr
      do m = 1, ntr
        Reg%Tr(m)%t => tracers(:,:,:,m) ; Reg%Tr(m)%conc_underflow = conc_underflow(m)
        write(tag, '(i0)') m
        Reg%Tr(m)%id_dfxy_cont = register_diag_field("ocean_model", "dfxy_cont_"//trim(tag), axes, Time)
        Reg%Tr(m)%id_dfx_2d = register_diag_field("ocean_model", "dfx_2d_"//trim(tag), axes, Time)
        Reg%Tr(m)%id_dfy_2d = register_diag_field("ocean_model", "dfy_2d_"//trim(tag), axes, Time)
      enddo
      allocate(Coef_x(ni_mem, nj_mem, nk+1), Coef_y(ni_mem, nj_mem, nk+1))
      Coef_x(:,:,:) = ieee_value(dt, ieee_quiet_nan) ; Coef_y(:,:,:) = ieee_value(dt, ieee_quiet_nan)
      Coef_x(:,:,1) = Coef_x1(:,:) ; Coef_y(:,:,1) = Coef_y1(:,:)
      p_ps => NULL()
      if (c_associated(p_surf)) call c_f_pointer(p_surf, p_ps, (/ int(ni_mem), int(nj_mem), int(ncalls) /))
      do r = 1, ncalls
        if (associated(p_ps)) then
          call neutral_diffusion_calc_coeffs(G, GV, US, h(:,:,:,r), T(:,:,:,r), S(:,:,:,r), visc, CS, p_surf=p_ps(:,:,r))
        else
          call neutral_diffusion_calc_coeffs(G, GV, US, h(:,:,:,r), T(:,:,:,r), S(:,:,:,r), visc, CS)
        endif
        call neutral_diffusion(G, GV, h(:,:,:,r), Coef_x, Coef_y, dt, Reg, US, CS)
      enddo
      deallocate(Reg%Tr) ; deallocate(Reg)
    endif
    call neutral_diffusion_end(CS)
    deallocate(diabatic_CSp) ; deallocate(G%Domain)
    call unit_scaling_end(US)
    ref_neutral_diffusion = standin_fatal_count
  end function

  ! ---- the lateral modules: MOM_lateral_mixing_coeffs.F90 (with MOM_isopycnal_slopes.F90) and MOM_thickness_diffuse.F90 ----
  !> The grid and vertical-grid members the lateral modules read beyond setup's.  metrics [18, nj_mem, ni_mem] holds, in this
  !! order, mask2dT, mask2dCu, mask2dCv, IdxCu, IdyCu, IdxCv, IdyCv, dxCu, dyCu, dxCv, dyCv, dy_Cu, dx_Cv, areaT, IareaT, areaCu,
  !! areaCv, bathyT; OBCmaskCu and OBCmaskCv are the face masks (no open boundaries).  vgx = (g_Earth, m2_s_to_HZ_T, H_to_kg_m2,
  !! max_depth).  dxT, dyT, dxBu, dyBu and Coriolis2Bu, which only the resolution-function part of VarMix_init reads (with
  !! USE_MEKE or a RESOLN_SCALED_ switch: tried for what the init refuses, never compared), are zero; dF_dx and dF_dy, which only
  !! calc_QG_Leith_viscosity reads, stay unallocated.
  subroutine setup_lateral(ni_mem, nj_mem, nk, vgx, metrics, Rlay, g_prime, G, GV)
    integer, intent(in) :: ni_mem, nj_mem, nk ; real, intent(in) :: vgx(4), metrics(ni_mem, nj_mem, 18), Rlay(nk), g_prime(nk+1)
    type(ocean_grid_type), intent(inout) :: G ; type(verticalGrid_type), intent(inout) :: GV
    allocate(G%mask2dCu(ni_mem, nj_mem), G%mask2dCv(ni_mem, nj_mem), G%OBCmaskCu(ni_mem, nj_mem), G%OBCmaskCv(ni_mem, nj_mem), &
             G%IdxCu(ni_mem, nj_mem), G%IdyCu(ni_mem, nj_mem), G%IdxCv(ni_mem, nj_mem), G%IdyCv(ni_mem, nj_mem), &
             G%dxCu(ni_mem, nj_mem), G%dyCu(ni_mem, nj_mem), G%dxCv(ni_mem, nj_mem), G%dyCv(ni_mem, nj_mem), &
             G%dy_Cu(ni_mem, nj_mem), G%dx_Cv(ni_mem, nj_mem), G%areaT(ni_mem, nj_mem), G%IareaT(ni_mem, nj_mem), &
             G%areaCu(ni_mem, nj_mem), G%areaCv(ni_mem, nj_mem), G%bathyT(ni_mem, nj_mem), G%Domain, &
             G%dxT(ni_mem, nj_mem), G%dyT(ni_mem, nj_mem), G%dxBu(ni_mem, nj_mem), G%dyBu(ni_mem, nj_mem), G%Coriolis2Bu(ni_mem, nj_mem))
    G%dxT(:,:) = 0.0 ; G%dyT(:,:) = 0.0 ; G%dxBu(:,:) = 0.0 ; G%dyBu(:,:) = 0.0 ; G%Coriolis2Bu(:,:) = 0.0
    G%mask2dCu(:,:) = metrics(:,:,2) ; G%mask2dCv(:,:) = metrics(:,:,3) ; G%OBCmaskCu(:,:) = metrics(:,:,2)
    G%OBCmaskCv(:,:) = metrics(:,:,3) ; G%IdxCu(:,:) = metrics(:,:,4) ; G%IdyCu(:,:) = metrics(:,:,5)
    G%IdxCv(:,:) = metrics(:,:,6) ; G%IdyCv(:,:) = metrics(:,:,7) ; G%dxCu(:,:) = metrics(:,:,8) ; G%dyCu(:,:) = metrics(:,:,9)
    G%dxCv(:,:) = metrics(:,:,10) ; G%dyCv(:,:) = metrics(:,:,11) ; G%dy_Cu(:,:) = metrics(:,:,12) ; G%dx_Cv(:,:) = metrics(:,:,13)
    G%areaT(:,:) = metrics(:,:,14) ; G%IareaT(:,:) = metrics(:,:,15) ; G%areaCu(:,:) = metrics(:,:,16)
    G%areaCv(:,:) = metrics(:,:,17) ; G%bathyT(:,:) = metrics(:,:,18) ; G%Z_ref = 0.0 ; G%ke = nk
    GV%g_Earth = vgx(1) ; GV%m2_s_to_HZ_T = vgx(2) ; GV%H_to_kg_m2 = vgx(3) ; GV%max_depth = vgx(4)
    GV%semi_Boussinesq = .false. ; GV%nkml = 0 ; GV%nk_rho_varies = 0
    allocate(GV%Rlay(nk), GV%g_prime(nk+1)) ; GV%Rlay(:) = Rlay(:) ; GV%g_prime(:) = g_prime(:)
  end subroutine setup_lateral

  !> unit_scaling_init, EOS_init (where T and S are given) and VarMix_init (MOM_lateral_mixing_coeffs.F90:1445) through the table,
  !! then calc_slope_functions (:686) `ncalls` times on the same VarMix_CS, on a whole tile.  h is [ncalls, nk, nj_mem, ni_mem]
  !! (round r reads slice r); T and S [nk, nj_mem, ni_mem] are C pointers, null together for "tv%eqn_of_state not associated" (the
  !! layered arm, which reads GV%Rlay); p_surf [nj_mem, ni_mem] is a C pointer, null for "not associated".  The OBC pointer is
  !! null.  Out come the public members CS%SN_u, CS%SN_v, CS%slope_x, CS%slope_y, CS%L2u, CS%L2v, each only where VarMix_init has
  !! allocated it (has = 1, else 0 and the array is left as it came); the diagnostics asked for with ref_want_diag (N2_u, N2_v,
  !! S2_u, S2_v, dzu_Visbeck, dzv_Visbeck, dzSxN, dzSyN, SN_u, SN_v, L2u, L2v) are read back with ref_get_diag.  No member of
  !! VarMix_CS is set from here.  dt <= 0: the inits only.
  integer(c_int) function ref_calc_slope_functions(ni_mem, nj_mem, idx, nk, vgr, vgx, metrics, Rlay, g_prime, ncalls, h, T, S, &
        p_surf, dt, SN_u, SN_v, slope_x, slope_y, L2u, L2v, has) bind(C, name="ref_calc_slope_functions")
    integer(c_int), value :: ni_mem, nj_mem, nk, ncalls ; integer(c_int), intent(in) :: idx(4)
    real(c_double), intent(in) :: vgr(14), vgx(4), metrics(ni_mem, nj_mem, 18), Rlay(nk), g_prime(nk+1)
    real(c_double), intent(inout) :: h(ni_mem, nj_mem, nk, ncalls) ; type(c_ptr), value :: T, S, p_surf ; real(c_double), value :: dt
    real(c_double), intent(inout), dimension(ni_mem, nj_mem) :: SN_u, SN_v, L2u, L2v
    real(c_double), intent(inout), dimension(ni_mem, nj_mem, nk+1) :: slope_x, slope_y
    integer(c_int), intent(out) :: has(3)
    type(ocean_grid_type) :: G ; type(verticalGrid_type) :: GV ; type(unit_scale_type), pointer :: US
    type(param_file_type) :: pf ; type(diag_ctrl), target :: diag ; type(time_type), target :: Time
    type(VarMix_CS) :: CS ; type(thermo_var_ptrs) :: tv ; type(EOS_type), target :: eqn ; type(ocean_OBC_type), pointer :: OBC
    integer :: r
    standin_fatal_count = 0 ; standin_never_count = 0 ; has(:) = 0
    call setup(int(ni_mem), int(nj_mem), int(idx), int(nk), vgr, metrics(:,:,1), c_null_ptr, pf, G, GV, US)
    call setup_lateral(int(ni_mem), int(nj_mem), int(nk), vgx, metrics, Rlay, g_prime, G, GV)
    if (c_associated(T) .and. c_associated(S)) then
      call c_f_pointer(T, tv%T, (/ int(ni_mem), int(nj_mem), int(nk) /))
      call c_f_pointer(S, tv%S, (/ int(ni_mem), int(nj_mem), int(nk) /))
      call EOS_init(pf, eqn, US) ; tv%eqn_of_state => eqn
    endif
    call plane(p_surf, int(ni_mem), int(nj_mem), tv%p_surf)
    call VarMix_init(Time, G, GV, US, pf, diag, CS)
    OBC => NULL()
    if (standin_fatal_count == 0 .and. dt > 0.0) then
      do r = 1, ncalls
        call calc_slope_functions(h(:,:,:,r), tv, dt, G, GV, US, CS, OBC)
      enddo
      if (allocated(CS%SN_u)) then ; has(1) = 1 ; SN_u(:,:) = CS%SN_u(:,:) ; SN_v(:,:) = CS%SN_v(:,:) ; endif
      if (allocated(CS%slope_x)) then ; has(2) = 1 ; slope_x(:,:,:) = CS%slope_x(:,:,:) ; slope_y(:,:,:) = CS%slope_y(:,:,:) ; endif
    endif
    if (allocated(CS%L2u)) then ; has(3) = 1 ; L2u(:,:) = CS%L2u(:,:) ; L2v(:,:) = CS%L2v(:,:) ; endif
    call VarMix_end(CS)
    deallocate(G%Domain)
    call unit_scaling_end(US)
    ref_calc_slope_functions = standin_fatal_count
  end function

  !> unit_scaling_init, EOS_init (where T and S are given), VarMix_init and thickness_diffuse_init (MOM_thickness_diffuse.F90:2170)
  !! through the table, then thickness_diffuse (:134) `ncalls` times on the same control structures, on a whole tile; h, uhtr and
  !! vhtr [nk, nj_mem, ni_mem] are changed in place, every round going on from the one before.  T, S, p_surf as in
  !! ref_calc_slope_functions.  The stored slopes go the reference's way, through VarMix%slope_x and VarMix%slope_y with
  !! VarMix%use_variable_mixing and VarMix%use_stored_slopes as VarMix_init sets them from USE_STORED_SLOPES (KHTH_SLOPE_CFF stays
  !! 0, so use_VarMix is false, :211):
  !!   mode 0: VarMix is as VarMix_init left it (no stored slopes unless the table asks for them, and then they are zero);
  !!   mode 1: slope_x and slope_y [nk + 1, nj_mem, ni_mem] are copied into the public members VarMix%slope_x and VarMix%slope_y,
  !!           which VarMix_init has allocated (the one member set from here: in the reference calc_slope_functions fills it);
  !!   mode 2: the chain: every round first calls calc_slope_functions on the same VarMix_CS with the round's h, whose stored slopes
  !!           thickness_diffuse then reads; slope_x, slope_y, SN_u and SN_v get the last round's.
  !! uhGM and vhGM get CDp%uhGM and CDp%vhGM where thickness_diffuse_init has allocated them (it does where ref_want_diag has
  !! asked for the diagnostics uhGM, vhGM: has = 1); the diagnostics asked for are read back with ref_get_diag.  MEKE is empty and
  !! STOCH has skeb_use_gm false.  dt <= 0: the inits only.
  integer(c_int) function ref_thickness_diffuse(ni_mem, nj_mem, idx, nk, vgr, vgx, metrics, Rlay, g_prime, ncalls, mode, h, uhtr, &
        vhtr, T, S, p_surf, dt, slope_x, slope_y, SN_u, SN_v, uhGM, vhGM, has) bind(C, name="ref_thickness_diffuse")
    integer(c_int), value :: ni_mem, nj_mem, nk, ncalls, mode ; integer(c_int), intent(in) :: idx(4)
    real(c_double), intent(in) :: vgr(14), vgx(4), metrics(ni_mem, nj_mem, 18), Rlay(nk), g_prime(nk+1)
    real(c_double), intent(inout), dimension(ni_mem, nj_mem, nk) :: h, uhtr, vhtr, uhGM, vhGM
    type(c_ptr), value :: T, S, p_surf ; real(c_double), value :: dt
    real(c_double), intent(inout), dimension(ni_mem, nj_mem, nk+1) :: slope_x, slope_y
    real(c_double), intent(inout), dimension(ni_mem, nj_mem) :: SN_u, SN_v
    integer(c_int), intent(out) :: has(2)
    type(ocean_grid_type) :: G ; type(verticalGrid_type) :: GV ; type(unit_scale_type), pointer :: US
    type(param_file_type) :: pf ; type(diag_ctrl), target :: diag ; type(time_type), target :: Time
    type(VarMix_CS) :: VarMix ; type(thickness_diffuse_CS) :: CS ; type(thermo_var_ptrs) :: tv ; type(EOS_type), target :: eqn
    type(ocean_OBC_type), pointer :: OBC ; type(MEKE_type) :: MEKE ; type(cont_diag_ptrs) :: CDp ; type(stochastic_CS) :: STOCH
    integer :: r
    standin_fatal_count = 0 ; standin_never_count = 0 ; has(:) = 0
    call setup(int(ni_mem), int(nj_mem), int(idx), int(nk), vgr, metrics(:,:,1), c_null_ptr, pf, G, GV, US)
    call setup_lateral(int(ni_mem), int(nj_mem), int(nk), vgx, metrics, Rlay, g_prime, G, GV)
    if (c_associated(T) .and. c_associated(S)) then
      call c_f_pointer(T, tv%T, (/ int(ni_mem), int(nj_mem), int(nk) /))
      call c_f_pointer(S, tv%S, (/ int(ni_mem), int(nj_mem), int(nk) /))
      call EOS_init(pf, eqn, US) ; tv%eqn_of_state => eqn
    endif
    call plane(p_surf, int(ni_mem), int(nj_mem), tv%p_surf)
    call VarMix_init(Time, G, GV, US, pf, diag, VarMix)
    call thickness_diffuse_init(Time, G, GV, US, pf, diag, CDp, CS)
    OBC => NULL() ; STOCH%skeb_use_gm = .false.
    if (mode == 1) then
      if (allocated(VarMix%slope_x) .and. allocated(VarMix%slope_y)) then
        VarMix%slope_x(:,:,:) = slope_x(:,:,:) ; VarMix%slope_y(:,:,:) = slope_y(:,:,:)
      else
        standin_fatal_count = standin_fatal_count + 1     ! the table of a stored-slopes case must set USE_STORED_SLOPES
      endif
    endif
    if (standin_fatal_count == 0 .and. dt > 0.0) then
      do r = 1, ncalls
        if (mode == 2) call calc_slope_functions(h, tv, dt, G, GV, US, VarMix, OBC)
        call thickness_diffuse(h, uhtr, vhtr, tv, dt, G, GV, US, MEKE, VarMix, CDp, CS, STOCH)
      enddo
      if (mode == 2) then
        slope_x(:,:,:) = VarMix%slope_x(:,:,:) ; slope_y(:,:,:) = VarMix%slope_y(:,:,:)
        SN_u(:,:) = VarMix%SN_u(:,:) ; SN_v(:,:) = VarMix%SN_v(:,:)
      endif
      if (associated(CDp%uhGM)) then ; has(1) = 1 ; uhGM(:,:,:) = CDp%uhGM(:,:,:) ; endif
      if (associated(CDp%vhGM)) then ; has(2) = 1 ; vhGM(:,:,:) = CDp%vhGM(:,:,:) ; endif
    endif
    call thickness_diffuse_end(CS, CDp)
    call VarMix_end(VarMix)
    deallocate(G%Domain)
    call unit_scaling_end(US)
    ref_thickness_diffuse = standin_fatal_count
  end function
end module ref_param_shim
