!> oracle/ref_standins.F90 -- ORACLE SUPPORT (test infrastructure only), not product and not reference text.
!!
!! The reference's parameterization modules (MOM_opacity.F90, MOM_energetic_PBL.F90, MOM_kappa_shear.F90,
!! MOM_neutral_diffusion.F90, MOM_isopycnal_slopes.F90, MOM_lateral_mixing_coeffs.F90, MOM_thickness_diffuse.F90) `use` framework modules
!! that need FMS and netCDF.  oracle/Makefile compiles those files, and every framework file that does compile on its own (the
!! equation-of-state dispatcher MOM_EOS.F90 with every module it uses among them), where they lie, against
!! the interface-only stand-ins below.  The rule is that of tests/fortran_stubs/mom_stubs.F90: each module carries the name of the
!! MOM6 module it stands for and declares ONLY the derived-type members and procedure signatures that the compiled reference files
!! touch (names, members and argument lists are interface facts); the bodies are a few lines of bookkeeping written here.
!!   * get_param answers from a name -> value table that the doors of ref_param_shim.F90 fill (standin_set_*), else with the
!!     call's default= or defaults=; log_param, log_version, openParameterBlock and closeParameterBlock do nothing;
!!   * register_diag_field returns a positive id for the names the door has asked for (standin_want_diag) and -1 otherwise;
!!     post_data copies the posted field into a store keyed by that id, which the door reads back (standin_get_diag);
!!   * query_averaging_enabled is true;
!!   * MOM_error(FATAL, ...) prints and counts (standin_fatal_count); it never stops, since a stop would end the test process;
!!   * EFP sums are plain sums (they feed a debugging printout only);
!!   * gsw_mod_toolbox (the TEOS-10 toolbox, a package the reference links to and does not hold) has the ten procedures that
!!     MOM_EOS_TEOS10.F90 and MOM_TFreeze.F90 name, which answer NaN: with it those two files and MOM_EOS.F90 compile from their own
!!     text.  No compared case selects TEOS10 or a TEOS10 freezing point, so none of the ten is ever called.
!!   * a procedure that no compared path may reach (pass_var, the procedures of MOM_remapping, MOM_hor_bnd_diffusion,
!!     MOM_CVMix_KPP and MOM_diabatic_driver, which MOM_neutral_diffusion.F90 names on its discontinuous, interior-only and
!!     vertical-structure paths; pass_vector, MOM_read_data and the two procedures of MOM_wave_speed, which the lateral modules
!!     name for calc_resoln_function, READ_KHTH and the resolution-function part of VarMix_init) calls standin_never: a FATAL,
!!     counted apart in standin_never_count.
!!   * MOM_open_boundary has the type, its members and the constants that MOM_isopycnal_slopes.F90 and
!!     MOM_lateral_mixing_coeffs.F90 name, and no procedure: the doors leave the OBC pointer null.
!! Stood in for: MOM_error_handler, MOM_coms, MOM_cpu_clock, MOM_time_manager, MOM_hor_index, MOM_domains, MOM_grid,
!! MOM_verticalGrid, MOM_file_parser, MOM_io (stdout, stderr, MOM_read_data, slasher), gsw_mod_toolbox, MOM_variables,
!! MOM_forcing_type, MOM_diag_mediator, MOM_debugging, MOM_wave_interface, MOM_stochastics, MOM_remapping, MOM_tracer_registry,
!! MOM_hor_bnd_diffusion, MOM_open_boundary, MOM_wave_speed, MOM_CVMix_KPP, MOM_diabatic_driver.  MOM_EOS and
!! MOM_interface_heights are no longer among them: the reference's own files are compiled.
!! The file is compiled three times: what needs neither a unit_scale_type nor an EOS_type before the reference's own
!! MOM_unit_scaling.F90 and equation-of-state files; MOM_variables (whose thermo_var_ptrs holds an EOS_type),
!! MOM_wave_speed, MOM_wave_interface and MOM_CVMix_KPP after them, with -DSTANDINS_AFTER_UNIT_SCALING; and
!! MOM_diabatic_driver (whose extract_diabatic_member names an energetic_PBL_CS) after the reference's MOM_energetic_PBL.F90,
!! with -DSTANDINS_AFTER_ENERGETIC_PBL as well.
#ifndef STANDINS_AFTER_UNIT_SCALING

module MOM_error_handler
  implicit none ; public
  integer, parameter :: NOTE = 0, WARNING = 1, FATAL = 2
  integer :: standin_fatal_count = 0     !< FATAL messages since the door last cleared it
  integer :: standin_never_count = 0     !< of those, the ones a stand-in procedure that must never run has raised
  logical :: standin_print_warnings = .false.
contains
  subroutine MOM_error(level, message, all_print)
    integer, intent(in) :: level ; character(len=*), intent(in) :: message ; logical, optional, intent(in) :: all_print
    if (level == FATAL) then
      standin_fatal_count = standin_fatal_count + 1
      print '(a)', "FATAL (counted, not stopped): "//trim(message) ; flush(6)
    elseif (level == WARNING .and. standin_print_warnings) then
      print '(a)', "WARNING: "//trim(message)
    endif
  end subroutine MOM_error
  subroutine MOM_mesg(message, verb, all_print)
    character(len=*), intent(in) :: message ; integer, optional, intent(in) :: verb ; logical, optional, intent(in) :: all_print
  end subroutine MOM_mesg
  logical function is_root_pe()
    is_root_pe = .true.
  end function is_root_pe
  !> What a stand-in procedure that must never run calls: it counts as a FATAL, and is counted apart, so that a door can tell a
  !! stop of the reference's own from a path that leads out of the compiled files.
  subroutine standin_never(who)
    character(len=*), intent(in) :: who
    standin_never_count = standin_never_count + 1
    call MOM_error(FATAL, "the stand-in "//trim(who)//" has been called: this path leaves the compiled reference files")
  end subroutine standin_never
end module MOM_error_handler

module MOM_coms
  implicit none ; private
  public :: EFP_type, real_to_EFP, EFP_to_real, EFP_sum_across_PEs, operator(+), assignment(=)
  type :: EFP_type ; real :: v = 0.0 ; end type EFP_type   ! a plain sum: it feeds only a debugging printout
  interface operator (+) ; module procedure EFP_plus ; end interface
  interface assignment(=) ; module procedure EFP_assign ; end interface
contains
  function EFP_plus(EFP1, EFP2)
    type(EFP_type) :: EFP_plus ; type(EFP_type), intent(in) :: EFP1, EFP2
    EFP_plus%v = EFP1%v + EFP2%v
  end function EFP_plus
  subroutine EFP_assign(EFP1, EFP2)
    type(EFP_type), intent(out) :: EFP1 ; type(EFP_type), intent(in) :: EFP2
    EFP1%v = EFP2%v
  end subroutine EFP_assign
  function real_to_EFP(val, overflow)
    real, intent(in) :: val ; logical, optional, intent(inout) :: overflow ; type(EFP_type) :: real_to_EFP
    real_to_EFP%v = val
  end function real_to_EFP
  function EFP_to_real(EFP1)
    type(EFP_type), intent(inout) :: EFP1 ; real :: EFP_to_real
    EFP_to_real = EFP1%v
  end function EFP_to_real
  subroutine EFP_sum_across_PEs(EFPs, nval, errors)
    type(EFP_type), dimension(:), intent(inout) :: EFPs ; integer, intent(in) :: nval
    logical, dimension(:), optional, intent(out) :: errors
    if (present(errors)) errors(:) = .false.
  end subroutine EFP_sum_across_PEs
end module MOM_coms

module MOM_cpu_clock
  implicit none ; public
  integer, parameter :: CLOCK_COMPONENT = 1, CLOCK_SUBCOMPONENT = 11, CLOCK_MODULE_DRIVER = 21, CLOCK_MODULE = 31, CLOCK_ROUTINE = 41
contains
  integer function cpu_clock_id(name, grain)
    character(len=*), intent(in) :: name ; integer, optional, intent(in) :: grain
    cpu_clock_id = 1
  end function cpu_clock_id
  subroutine cpu_clock_begin(id) ; integer, intent(in) :: id ; end subroutine
  subroutine cpu_clock_end(id) ; integer, intent(in) :: id ; end subroutine
end module MOM_cpu_clock

module MOM_time_manager
  implicit none ; public
  type :: time_type ; integer :: seconds = 0, days = 0 ; end type time_type
end module MOM_time_manager

module MOM_hor_index
  implicit none ; public
  type :: hor_index_type
    integer :: isc, iec, jsc, jec, isd, ied, jsd, jed, IscB, IecB, JscB, JecB, IsdB, IedB, JsdB, JedB
    integer :: idg_offset = 0, jdg_offset = 0
    logical :: symmetric = .true.
  end type hor_index_type
end module MOM_hor_index

module MOM_domains
  use MOM_error_handler, only : standin_never
  implicit none ; public
  type :: MOM_domain_type ; integer :: dummy = 0 ; end type MOM_domain_type
  type :: group_pass_type ; integer :: dummy = 0 ; end type group_pass_type
  integer, parameter :: CORNER = 1      ! (the stand-in tells nothing by it)
  interface pass_var
    module procedure pass_var_2d, pass_var_3d
  end interface
  interface pass_vector
    module procedure pass_vector_2d, pass_vector_3d
  end interface
contains
  !> Never reached: MOM_lateral_mixing_coeffs.F90 and MOM_thickness_diffuse.F90 import the name and do not call it.
  subroutine pass_vector_2d(u_cmpt, v_cmpt, MOM_dom, direction, stagger, complete, halo, clock)
    real, dimension(:,:), intent(inout) :: u_cmpt, v_cmpt ; type(MOM_domain_type), intent(inout) :: MOM_dom
    integer, optional, intent(in) :: direction, stagger, halo, clock ; logical, optional, intent(in) :: complete
    call standin_never("pass_vector (2-D)")
  end subroutine pass_vector_2d
  subroutine pass_vector_3d(u_cmpt, v_cmpt, MOM_dom, direction, stagger, complete, halo, clock)
    real, dimension(:,:,:), intent(inout) :: u_cmpt, v_cmpt ; type(MOM_domain_type), intent(inout) :: MOM_dom
    integer, optional, intent(in) :: direction, stagger, halo, clock ; logical, optional, intent(in) :: complete
    call standin_never("pass_vector (3-D)")
  end subroutine pass_vector_3d
  !> Never reached: MOM_neutral_diffusion passes the boundary-layer depth (NDIFF_INTERIOR_ONLY) and Coef_h (KHTR_USE_EBT_STRUCT),
  !! both of which the device refuses; calc_resoln_function and calc_sqg_struct (not compared) pass their structure functions, and
  !! thickness_diffuse_init the khth2d plane it has read (READ_KHTH, left out of the comparison).
  subroutine pass_var_2d(array, MOM_dom, sideflag, complete, position, halo, inner_halo, clock)
    real, dimension(:,:), intent(inout) :: array ; type(MOM_domain_type), intent(inout) :: MOM_dom
    integer, optional, intent(in) :: sideflag, position, halo, inner_halo, clock ; logical, optional, intent(in) :: complete
    call standin_never("pass_var (2-D)")
  end subroutine pass_var_2d
  subroutine pass_var_3d(array, MOM_dom, sideflag, complete, position, halo, inner_halo, clock)
    real, dimension(:,:,:), intent(inout) :: array ; type(MOM_domain_type), intent(inout) :: MOM_dom
    integer, optional, intent(in) :: sideflag, position, halo, inner_halo, clock ; logical, optional, intent(in) :: complete
    call standin_never("pass_var (3-D)")
  end subroutine pass_var_3d
  !> Bookkeeping only, as before.  do_group_pass is never reached: ePBL's group stays unused and calc_resoln_function, which
  !! passes cg1, is not compared.
  subroutine create_group_pass(group, array, MOM_dom)
    type(group_pass_type), intent(inout) :: group ; real, dimension(:,:), intent(inout) :: array
    type(MOM_domain_type), intent(inout) :: MOM_dom
  end subroutine create_group_pass
  subroutine do_group_pass(group, MOM_dom)
    type(group_pass_type), intent(inout) :: group ; type(MOM_domain_type), intent(inout) :: MOM_dom
  end subroutine do_group_pass
end module MOM_domains

module MOM_grid
  use MOM_hor_index, only : hor_index_type
  use MOM_domains, only : MOM_domain_type
  implicit none ; public
  type :: ocean_grid_type
    type(hor_index_type) :: HI
    type(MOM_domain_type), pointer :: Domain => NULL()
    integer :: isc, iec, jsc, jec, isd, ied, jsd, jed, IscB, IecB, JscB, JecB, IsdB, IedB, JsdB, JedB, ke
    real, allocatable, dimension(:,:) :: mask2dT, CoriolisBu, geoLonT, geoLatT, Coriolis2Bu, mask2dCu, mask2dCv, mask2dBu, IareaT
    real, allocatable, dimension(:,:) :: OBCmaskCu, OBCmaskCv, areaT, areaCu, areaCv, bathyT, dF_dx, dF_dy
    real, allocatable, dimension(:,:) :: dxT, dyT, dxCu, dyCu, dxCv, dyCv, dxBu, dyBu, IdxCu, IdyCu, IdxCv, IdyCv, dx_Cv, dy_Cu
    real :: Z_ref = 0.0
  end type ocean_grid_type
end module MOM_grid

module MOM_verticalGrid
  implicit none ; public
  type :: verticalGrid_type
    integer :: ke, nkml = 0
    logical :: Boussinesq = .true., semi_Boussinesq = .false.
    real :: Rho0, g_Earth, g_Earth_Z_T2, Angstrom_H, Angstrom_Z, H_subroundoff, dZ_subroundoff
    real :: H_to_Z = 1., Z_to_H = 1., H_to_RZ, RZ_to_H, H_to_m = 1., m_to_H = 1., H_to_MKS = 1., HZ_T_to_m2_s = 1.
    real :: m2_s_to_HZ_T = 1., HZ_T_to_MKS = 1., H_to_pa = 1., kg_m2_to_H = 1., H_to_kg_m2 = 1., max_depth = 0.
    integer :: nk_rho_varies = 0
    real, allocatable, dimension(:) :: Rlay, g_prime
  end type verticalGrid_type
end module MOM_verticalGrid

module MOM_file_parser
  implicit none ; private
  public :: param_file_type, get_param, log_param, log_version, openParameterBlock, closeParameterBlock
  public :: standin_clear_params, standin_set_real, standin_set_int, standin_set_char, standin_set_reals
  type :: param_file_type ; integer :: dummy = 0 ; end type param_file_type
  integer, parameter :: NMAX = 256, AMAX = 32
  !> the name -> value table the doors fill: one table for the process (the doors run one at a time)
  integer :: ntab = 0
  character(len=64) :: tab_name(NMAX) = ""
  character(len=128) :: tab_char(NMAX) = ""
  integer :: tab_int(NMAX) = 0, tab_len(NMAX) = 0
  real :: tab_real(AMAX, NMAX) = 0.0
  interface get_param
    module procedure get_param_real, get_param_int, get_param_logical, get_param_char, get_param_real_array
  end interface
  interface log_param
    module procedure log_param_real, log_param_char
  end interface
contains
  subroutine standin_clear_params()
    ntab = 0
  end subroutine standin_clear_params
  integer function slot(name)
    character(len=*), intent(in) :: name ; integer :: m
    do m = 1, ntab ; if (trim(tab_name(m)) == trim(name)) then ; slot = m ; return ; endif ; enddo
    ntab = ntab + 1 ; slot = ntab ; tab_name(ntab) = name ; tab_len(ntab) = 0 ; tab_char(ntab) = "" ; tab_int(ntab) = 0
  end function slot
  integer function find(name)
    character(len=*), intent(in) :: name ; integer :: m
    find = 0
    do m = 1, ntab ; if (trim(tab_name(m)) == trim(name)) then ; find = m ; return ; endif ; enddo
  end function find
  subroutine standin_set_real(name, value)
    character(len=*), intent(in) :: name ; real, intent(in) :: value ; integer :: m
    m = slot(name) ; tab_real(1, m) = value ; tab_len(m) = 1
  end subroutine standin_set_real
  subroutine standin_set_reals(name, values)
    character(len=*), intent(in) :: name ; real, intent(in) :: values(:) ; integer :: m
    m = slot(name) ; tab_len(m) = min(size(values), AMAX) ; tab_real(1:tab_len(m), m) = values(1:tab_len(m))
  end subroutine standin_set_reals
  subroutine standin_set_int(name, value)   ! (logicals too: 0 is false)
    character(len=*), intent(in) :: name ; integer, intent(in) :: value ; integer :: m
    m = slot(name) ; tab_int(m) = value
  end subroutine standin_set_int
  subroutine standin_set_char(name, value)
    character(len=*), intent(in) :: name, value ; integer :: m
    m = slot(name) ; tab_char(m) = value
  end subroutine standin_set_char

  subroutine get_param_real(CS, modulename, varname, value, desc, units, default, fail_if_missing, do_not_read, do_not_log, &
                            debuggingParam, scale, unscaled, layoutParam, old_name)
    type(param_file_type), intent(in) :: CS ; character(len=*), intent(in) :: modulename, varname
    real, intent(inout) :: value ; character(len=*), optional, intent(in) :: desc, units, old_name
    real, optional, intent(in) :: default, scale ; real, optional, intent(out) :: unscaled
    logical, optional, intent(in) :: fail_if_missing, do_not_read, do_not_log, debuggingParam, layoutParam
    integer :: m
    m = find(varname)
    if (m > 0) then ; value = tab_real(1, m)
    elseif (present(default)) then ; value = default ; endif
    if (present(unscaled)) unscaled = value
    if (present(scale)) value = scale * value
  end subroutine get_param_real
  subroutine get_param_real_array(CS, modulename, varname, value, desc, units, default, defaults, fail_if_missing, do_not_read, &
                                  do_not_log, debuggingParam, scale, unscaled, old_name)
    type(param_file_type), intent(in) :: CS ; character(len=*), intent(in) :: modulename, varname
    real, dimension(:), intent(inout) :: value ; character(len=*), optional, intent(in) :: desc, units, old_name
    real, optional, intent(in) :: default, scale ; real, dimension(:), optional, intent(in) :: defaults
    real, dimension(:), optional, intent(out) :: unscaled
    logical, optional, intent(in) :: fail_if_missing, do_not_read, do_not_log, debuggingParam
    integer :: m, n
    m = find(varname)
    if (m > 0) then
      n = min(size(value), tab_len(m)) ; value(1:n) = tab_real(1:n, m)
    elseif (present(defaults)) then
      n = min(size(value), size(defaults)) ; value(1:n) = defaults(1:n)
    elseif (present(default)) then ; value(:) = default ; endif
    if (present(unscaled)) unscaled(:) = value(:)
    if (present(scale)) value(:) = scale * value(:)
  end subroutine get_param_real_array
  subroutine get_param_int(CS, modulename, varname, value, desc, units, default, fail_if_missing, do_not_read, do_not_log, &
                           debuggingParam, layoutParam, old_name)
    type(param_file_type), intent(in) :: CS ; character(len=*), intent(in) :: modulename, varname
    integer, intent(inout) :: value ; character(len=*), optional, intent(in) :: desc, units, old_name
    integer, optional, intent(in) :: default
    logical, optional, intent(in) :: fail_if_missing, do_not_read, do_not_log, debuggingParam, layoutParam
    integer :: m
    m = find(varname)
    if (m > 0) then ; value = tab_int(m)
    elseif (present(default)) then ; value = default ; endif
  end subroutine get_param_int
  subroutine get_param_logical(CS, modulename, varname, value, desc, units, default, fail_if_missing, do_not_read, do_not_log, &
                               debuggingParam, layoutParam, old_name)
    type(param_file_type), intent(in) :: CS ; character(len=*), intent(in) :: modulename, varname
    logical, intent(inout) :: value ; character(len=*), optional, intent(in) :: desc, units, old_name
    logical, optional, intent(in) :: default
    logical, optional, intent(in) :: fail_if_missing, do_not_read, do_not_log, debuggingParam, layoutParam
    integer :: m
    m = find(varname)
    if (m > 0) then ; value = (tab_int(m) /= 0)
    elseif (present(default)) then ; value = default ; endif
  end subroutine get_param_logical
  subroutine get_param_char(CS, modulename, varname, value, desc, units, default, fail_if_missing, do_not_read, do_not_log, &
                            debuggingParam, layoutParam, old_name)
    type(param_file_type), intent(in) :: CS ; character(len=*), intent(in) :: modulename, varname
    character(len=*), intent(inout) :: value ; character(len=*), optional, intent(in) :: desc, units, default, old_name
    logical, optional, intent(in) :: fail_if_missing, do_not_read, do_not_log, debuggingParam, layoutParam
    integer :: m
    m = find(varname)
    if (m > 0) then ; value = trim(tab_char(m))
    elseif (present(default)) then ; value = default ; endif
  end subroutine get_param_char

  subroutine log_param_real(CS, modulename, varname, value, desc, units, default, debuggingParam, like_default, unscale)
    type(param_file_type), intent(in) :: CS ; character(len=*), intent(in) :: modulename, varname ; real, intent(in) :: value
    character(len=*), optional, intent(in) :: desc, units ; real, optional, intent(in) :: default, unscale
    logical, optional, intent(in) :: debuggingParam, like_default
  end subroutine log_param_real
  subroutine log_param_char(CS, modulename, varname, value, desc, units, default, layoutParam, debuggingParam, like_default)
    type(param_file_type), intent(in) :: CS ; character(len=*), intent(in) :: modulename, varname, value
    character(len=*), optional, intent(in) :: desc, units, default ; logical, optional, intent(in) :: layoutParam, debuggingParam, like_default
  end subroutine log_param_char
  subroutine log_version(CS, modulename, version, desc, all_default, layout, debugging, log_to_all)
    type(param_file_type), intent(in) :: CS ; character(len=*), intent(in) :: modulename, version
    character(len=*), optional, intent(in) :: desc ; logical, optional, intent(in) :: all_default, layout, debugging, log_to_all
  end subroutine log_version
  subroutine openParameterBlock(CS, blockName, desc, do_not_log)
    type(param_file_type), intent(in) :: CS ; character(len=*), intent(in) :: blockName
    character(len=*), optional, intent(in) :: desc ; logical, optional, intent(in) :: do_not_log
  end subroutine openParameterBlock
  subroutine closeParameterBlock(CS)
    type(param_file_type), intent(in) :: CS
  end subroutine closeParameterBlock
end module MOM_file_parser

module MOM_io
  use, intrinsic :: iso_fortran_env, only : stdout => output_unit, stderr => error_unit
  use MOM_error_handler, only : standin_never
  use MOM_domains, only : MOM_domain_type
  implicit none ; public
contains
  !> Never reached: only thickness_diffuse_init with READ_KHTH reads a file, and that case is left out of the comparison (the
  !! plane it reads lands in a private member).  The data come back zero.
  subroutine MOM_read_data(filename, fieldname, data, MOM_Domain, timelevel, position, scale)
    character(len=*), intent(in) :: filename, fieldname ; real, dimension(:,:), intent(inout) :: data
    type(MOM_domain_type), intent(in) :: MOM_Domain ; integer, optional, intent(in) :: timelevel, position
    real, optional, intent(in) :: scale
    data(:,:) = 0.0
    call standin_never("MOM_read_data")
  end subroutine MOM_read_data
  !> The directory name with one slash at its end (a string helper: it reads nothing).
  function slasher(dir)
    character(len=*), intent(in) :: dir ; character(len=len(dir)+2) :: slasher
    slasher = trim(dir)
    if (len_trim(dir) > 0) then ; if (dir(len_trim(dir):len_trim(dir)) /= "/") slasher = trim(dir)//"/" ; endif
  end function slasher
end module MOM_io

module gsw_mod_toolbox
  use, intrinsic :: ieee_arithmetic, only : ieee_value, ieee_quiet_nan
  implicit none ; private
  public :: gsw_sp_from_sr, gsw_sr_from_sp, gsw_pt_from_ct, gsw_ct_from_pt, gsw_rho, gsw_specvol, gsw_ct_freezing_exact
  public :: gsw_rho_first_derivatives, gsw_rho_second_derivatives, gsw_specvol_first_derivatives
contains
  elemental real function gsw_sp_from_sr(sr) ; real, intent(in) :: sr
    gsw_sp_from_sr = ieee_value(sr, ieee_quiet_nan) ; end function
  elemental real function gsw_sr_from_sp(sp) ; real, intent(in) :: sp
    gsw_sr_from_sp = ieee_value(sp, ieee_quiet_nan) ; end function
  elemental real function gsw_pt_from_ct(sa, ct) ; real, intent(in) :: sa, ct
    gsw_pt_from_ct = ieee_value(sa, ieee_quiet_nan) ; end function
  elemental real function gsw_ct_from_pt(sa, pt) ; real, intent(in) :: sa, pt
    gsw_ct_from_pt = ieee_value(sa, ieee_quiet_nan) ; end function
  elemental real function gsw_rho(sa, ct, p) ; real, intent(in) :: sa, ct, p
    gsw_rho = ieee_value(sa, ieee_quiet_nan) ; end function
  elemental real function gsw_specvol(sa, ct, p) ; real, intent(in) :: sa, ct, p
    gsw_specvol = ieee_value(sa, ieee_quiet_nan) ; end function
  elemental real function gsw_ct_freezing_exact(sa, p, saturation_fraction) ; real, intent(in) :: sa, p, saturation_fraction
    gsw_ct_freezing_exact = ieee_value(sa, ieee_quiet_nan) ; end function
  elemental subroutine gsw_rho_first_derivatives(sa, ct, p, drho_dsa, drho_dct, drho_dp)
    real, intent(in) :: sa, ct, p ; real, intent(out), optional :: drho_dsa, drho_dct, drho_dp
    if (present(drho_dsa)) drho_dsa = ieee_value(sa, ieee_quiet_nan)
    if (present(drho_dct)) drho_dct = ieee_value(sa, ieee_quiet_nan)
    if (present(drho_dp)) drho_dp = ieee_value(sa, ieee_quiet_nan)
  end subroutine
  elemental subroutine gsw_rho_second_derivatives(sa, ct, p, rho_sa_sa, rho_sa_ct, rho_ct_ct, rho_sa_p, rho_ct_p)
    real, intent(in) :: sa, ct, p ; real, intent(out), optional :: rho_sa_sa, rho_sa_ct, rho_ct_ct, rho_sa_p, rho_ct_p
    if (present(rho_sa_sa)) rho_sa_sa = ieee_value(sa, ieee_quiet_nan)
    if (present(rho_sa_ct)) rho_sa_ct = ieee_value(sa, ieee_quiet_nan)
    if (present(rho_ct_ct)) rho_ct_ct = ieee_value(sa, ieee_quiet_nan)
    if (present(rho_sa_p)) rho_sa_p = ieee_value(sa, ieee_quiet_nan)
    if (present(rho_ct_p)) rho_ct_p = ieee_value(sa, ieee_quiet_nan)
  end subroutine
  elemental subroutine gsw_specvol_first_derivatives(sa, ct, p, v_sa, v_ct, v_p)
    real, intent(in) :: sa, ct, p ; real, intent(out), optional :: v_sa, v_ct, v_p
    if (present(v_sa)) v_sa = ieee_value(sa, ieee_quiet_nan)
    if (present(v_ct)) v_ct = ieee_value(sa, ieee_quiet_nan)
    if (present(v_p)) v_p = ieee_value(sa, ieee_quiet_nan)
  end subroutine
end module gsw_mod_toolbox

module MOM_forcing_type
  implicit none ; public
  type :: forcing
    real, pointer, dimension(:,:) :: ustar => NULL(), ustar_gustless => NULL(), tau_mag => NULL(), tau_mag_gustless => NULL(), &
                                     ustar_shelf => NULL(), frac_shelf_h => NULL(), BBL_tidal_dis => NULL()
  end type forcing
end module MOM_forcing_type

module MOM_diag_mediator
  use MOM_time_manager, only : time_type
  implicit none ; private
  public :: time_type, diag_ctrl, axes_grp, register_diag_field, post_data, query_averaging_enabled, safe_alloc_ptr, safe_alloc_alloc
  public :: diag_update_remap_grids
  public :: standin_clear_diags, standin_want_diag, standin_diag_size, standin_get_diag
  type :: axes_grp ; integer :: rank = 0 ; end type axes_grp
  type :: diag_ctrl
    type(axes_grp) :: axesT1, axesTL, axesTi, axesBi, axesCu1, axesCv1, axesCuL, axesCvL, axesCui, axesCvi
  end type diag_ctrl
  integer, parameter :: NDMAX = 64
  type :: capture ; real, allocatable :: v(:) ; end type capture
  !> the names the door has asked for; a field's id is its place in this list; what post_data last copied for it
  integer :: nwant = 0
  character(len=48) :: want_name(NDMAX) = ""
  type(capture) :: store(NDMAX)
  interface post_data
    module procedure post_data_2d, post_data_3d
  end interface
  interface safe_alloc_ptr
    module procedure safe_alloc_ptr_2d, safe_alloc_ptr_3d
  end interface
  interface safe_alloc_alloc
    module procedure safe_alloc_alloc_2d, safe_alloc_alloc_3d
  end interface
contains
  subroutine standin_clear_diags()
    integer :: m
    do m = 1, NDMAX ; if (allocated(store(m)%v)) deallocate(store(m)%v) ; enddo
    nwant = 0
  end subroutine standin_clear_diags
  subroutine standin_want_diag(name)
    character(len=*), intent(in) :: name
    if (nwant < NDMAX) then ; nwant = nwant + 1 ; want_name(nwant) = name ; endif
  end subroutine standin_want_diag
  integer function want_id(name)
    character(len=*), intent(in) :: name ; integer :: m
    want_id = -1
    do m = 1, nwant ; if (trim(want_name(m)) == trim(name)) then ; want_id = m ; return ; endif ; enddo
  end function want_id
  !> the number of values captured for a name: 0 when nothing was posted, -1 when the name was not asked for
  integer function standin_diag_size(name)
    character(len=*), intent(in) :: name ; integer :: m
    m = want_id(name) ; standin_diag_size = -1
    if (m > 0) then ; standin_diag_size = 0 ; if (allocated(store(m)%v)) standin_diag_size = size(store(m)%v) ; endif
  end function standin_diag_size
  subroutine standin_get_diag(name, out)
    character(len=*), intent(in) :: name ; real, intent(inout) :: out(:) ; integer :: m, n
    m = want_id(name) ; if (m < 1) return ; if (.not.allocated(store(m)%v)) return
    n = min(size(out), size(store(m)%v)) ; out(1:n) = store(m)%v(1:n)
  end subroutine standin_get_diag

  integer function register_diag_field(module_name, field_name, axes, init_time, long_name, units, conversion, cmor_long_name, &
                                       cmor_field_name, cmor_standard_name, x_cell_method, y_cell_method, v_extensive)
    character(len=*), intent(in) :: module_name, field_name ; type(axes_grp), intent(in) :: axes ; type(time_type), intent(in) :: init_time
    character(len=*), optional, intent(in) :: long_name, units, cmor_long_name ; real, optional, intent(in) :: conversion
    character(len=*), optional, intent(in) :: cmor_field_name, cmor_standard_name, x_cell_method, y_cell_method
    logical, optional, intent(in) :: v_extensive
    register_diag_field = want_id(field_name)
  end function register_diag_field
  !> Nothing to do: no diagnostic is remapped here.
  subroutine diag_update_remap_grids(diag_cs)
    type(diag_ctrl), intent(inout) :: diag_cs
  end subroutine diag_update_remap_grids
  subroutine post_data_2d(diag_field_id, field, diag_cs)
    integer, intent(in) :: diag_field_id ; real, intent(in) :: field(:,:) ; type(diag_ctrl), intent(in) :: diag_cs
    if (diag_field_id < 1 .or. diag_field_id > NDMAX) return
    if (allocated(store(diag_field_id)%v)) deallocate(store(diag_field_id)%v)
    allocate(store(diag_field_id)%v(size(field))) ; store(diag_field_id)%v(:) = reshape(field, (/ size(field) /))
  end subroutine post_data_2d
  subroutine post_data_3d(diag_field_id, field, diag_cs)
    integer, intent(in) :: diag_field_id ; real, intent(in) :: field(:,:,:) ; type(diag_ctrl), intent(in) :: diag_cs
    if (diag_field_id < 1 .or. diag_field_id > NDMAX) return
    if (allocated(store(diag_field_id)%v)) deallocate(store(diag_field_id)%v)
    allocate(store(diag_field_id)%v(size(field))) ; store(diag_field_id)%v(:) = reshape(field, (/ size(field) /))
  end subroutine post_data_3d
  logical function query_averaging_enabled(diag_cs)
    type(diag_ctrl), intent(in) :: diag_cs
    query_averaging_enabled = .true.
  end function query_averaging_enabled
  subroutine safe_alloc_ptr_2d(ptr, is, ie, js, je)
    real, dimension(:,:), pointer :: ptr ; integer, intent(in) :: is, ie, js, je
    if (.not.associated(ptr)) then ; allocate(ptr(is:ie,js:je)) ; ptr(:,:) = 0.0 ; endif
  end subroutine safe_alloc_ptr_2d
  subroutine safe_alloc_ptr_3d(ptr, is, ie, js, je, nk)
    real, dimension(:,:,:), pointer :: ptr ; integer, intent(in) :: is, ie, js, je, nk
    if (.not.associated(ptr)) then ; allocate(ptr(is:ie,js:je,nk)) ; ptr(:,:,:) = 0.0 ; endif
  end subroutine safe_alloc_ptr_3d
  subroutine safe_alloc_alloc_2d(ptr, is, ie, js, je)
    real, dimension(:,:), allocatable :: ptr ; integer, intent(in) :: is, ie, js, je
    if (.not.allocated(ptr)) then ; allocate(ptr(is:ie,js:je)) ; ptr(:,:) = 0.0 ; endif
  end subroutine safe_alloc_alloc_2d
  subroutine safe_alloc_alloc_3d(ptr, is, ie, js, je, nk)
    real, dimension(:,:,:), allocatable :: ptr ; integer, intent(in) :: is, ie, js, je, nk
    if (.not.allocated(ptr)) then ; allocate(ptr(is:ie,js:je,nk)) ; ptr(:,:,:) = 0.0 ; endif
  end subroutine safe_alloc_alloc_3d
end module MOM_diag_mediator

module MOM_debugging
  use MOM_hor_index, only : hor_index_type
  implicit none ; private
  public :: hchksum, Bchksum, uvchksum
  interface uvchksum
    module procedure uvchksum_2d, uvchksum_3d
  end interface
  interface hchksum
    module procedure hchksum_2d, hchksum_3d
  end interface
  interface Bchksum
    module procedure hchksum_2d, hchksum_3d
  end interface
contains
  subroutine hchksum_2d(array, mesg, HI, haloshift, unscale)
    real, intent(in) :: array(:,:) ; character(len=*), intent(in) :: mesg ; type(hor_index_type), intent(in) :: HI
    integer, optional, intent(in) :: haloshift ; real, optional, intent(in) :: unscale
  end subroutine hchksum_2d
  subroutine hchksum_3d(array, mesg, HI, haloshift, unscale)
    real, intent(in) :: array(:,:,:) ; character(len=*), intent(in) :: mesg ; type(hor_index_type), intent(in) :: HI
    integer, optional, intent(in) :: haloshift ; real, optional, intent(in) :: unscale
  end subroutine hchksum_3d
  subroutine uvchksum_2d(mesg, arrayU, arrayV, HI, haloshift, symmetric, omit_corners, unscale, logunit, scalar_pair)
    character(len=*), intent(in) :: mesg ; real, intent(in) :: arrayU(:,:), arrayV(:,:) ; type(hor_index_type), intent(in) :: HI
    integer, optional, intent(in) :: haloshift, logunit ; logical, optional, intent(in) :: symmetric, omit_corners, scalar_pair
    real, optional, intent(in) :: unscale
  end subroutine uvchksum_2d
  subroutine uvchksum_3d(mesg, arrayU, arrayV, HI, haloshift, symmetric, omit_corners, unscale, logunit, scalar_pair)
    character(len=*), intent(in) :: mesg ; real, intent(in) :: arrayU(:,:,:), arrayV(:,:,:) ; type(hor_index_type), intent(in) :: HI
    integer, optional, intent(in) :: haloshift, logunit ; logical, optional, intent(in) :: symmetric, omit_corners, scalar_pair
    real, optional, intent(in) :: unscale
  end subroutine uvchksum_3d
end module MOM_debugging

module MOM_stochastics
  implicit none ; public
  type :: stochastic_CS
    logical :: pert_epbl = .false., skeb_use_gm = .false.
    integer :: id_epbl1_wts = -1, id_epbl2_wts = -1
    real :: skeb_gm_coef = 0.0
    real, allocatable, dimension(:,:) :: epbl1_wts, epbl2_wts
    real, allocatable, dimension(:,:,:) :: skeb_diss
  end type stochastic_CS
end module MOM_stochastics


module MOM_remapping
  use MOM_error_handler, only : standin_never
  implicit none ; private
  public :: remapping_CS, initialize_remapping, extract_member_remapping_CS, build_reconstructions_1d, average_value_ppoly
  public :: remappingSchemesDoc, remappingDefaultScheme
  type :: remapping_CS ; integer :: degree = 0 ; end type remapping_CS
  character(len=*), parameter :: remappingSchemesDoc = "(MOM_remapping is stood in for: no scheme is known here)"
  character(len=*), parameter :: remappingDefaultScheme = "STOOD_IN_FOR"
contains
  !> Never reached by a compared case: only the discontinuous reconstruction (NDIFF_CONTINUOUS false, which the device refuses)
  !! sets up and uses a remapping control structure.
  subroutine initialize_remapping(CS, remapping_scheme, boundary_extrapolation, check_reconstruction, check_remapping, &
        force_bounds_in_subcell, force_bounds_in_target, better_force_bounds_in_target, offset_tgt_summation, &
        om4_remap_via_sub_cells, answers_2018, answer_date, nk, h_neglect, h_neglect_edge)
    type(remapping_CS), intent(inout) :: CS ; character(len=*), intent(in) :: remapping_scheme
    logical, optional, intent(in) :: boundary_extrapolation, check_reconstruction, check_remapping, force_bounds_in_subcell, &
                                     force_bounds_in_target, better_force_bounds_in_target, offset_tgt_summation, &
                                     om4_remap_via_sub_cells, answers_2018
    integer, optional, intent(in) :: answer_date, nk ; real, optional, intent(in) :: h_neglect, h_neglect_edge
    call standin_never("initialize_remapping")
  end subroutine initialize_remapping
  subroutine extract_member_remapping_CS(CS, remapping_scheme, degree, boundary_extrapolation, check_reconstruction, &
        check_remapping, force_bounds_in_subcell, force_bounds_in_target, better_force_bounds_in_target, offset_tgt_summation)
    type(remapping_CS), intent(in) :: CS ; integer, optional, intent(out) :: remapping_scheme, degree
    logical, optional, intent(out) :: boundary_extrapolation, check_reconstruction, check_remapping, force_bounds_in_subcell, &
                                      force_bounds_in_target, better_force_bounds_in_target, offset_tgt_summation
    if (present(remapping_scheme)) remapping_scheme = 0
    if (present(degree)) degree = CS%degree
    if (present(boundary_extrapolation)) boundary_extrapolation = .false.
    if (present(check_reconstruction)) check_reconstruction = .false.
    if (present(check_remapping)) check_remapping = .false.
    if (present(force_bounds_in_subcell)) force_bounds_in_subcell = .false.
    if (present(force_bounds_in_target)) force_bounds_in_target = .false.
    if (present(better_force_bounds_in_target)) better_force_bounds_in_target = .false.
    if (present(offset_tgt_summation)) offset_tgt_summation = .false.
    call standin_never("extract_member_remapping_CS")
  end subroutine extract_member_remapping_CS
  subroutine build_reconstructions_1d(CS, n0, h0, u0, ppoly_r_coefs, ppoly_r_E, ppoly_r_S, iMethod, h_neglect, h_neglect_edge, &
                                      PCM_cell, debug)
    type(remapping_CS), intent(in) :: CS ; integer, intent(in) :: n0 ; real, dimension(n0), intent(in) :: h0, u0
    real, dimension(:,:), intent(out) :: ppoly_r_coefs ; real, dimension(n0,2), intent(out) :: ppoly_r_E, ppoly_r_S
    integer, intent(out) :: iMethod ; real, intent(in) :: h_neglect ; real, optional, intent(in) :: h_neglect_edge
    logical, optional, intent(in) :: PCM_cell(n0), debug
    ppoly_r_coefs(:,:) = 0.0 ; ppoly_r_E(:,:) = 0.0 ; ppoly_r_S(:,:) = 0.0 ; iMethod = 0
    call standin_never("build_reconstructions_1d")
  end subroutine build_reconstructions_1d
  real function average_value_ppoly(n0, u0, ppoly0_E, ppoly0_coefs, method, i0, xa, xb)
    integer, intent(in) :: n0, method, i0 ; real, intent(in) :: u0(n0), ppoly0_E(n0,2), ppoly0_coefs(:,:), xa, xb
    average_value_ppoly = 0.0
    call standin_never("average_value_ppoly")
  end function average_value_ppoly
end module MOM_remapping

module MOM_tracer_registry
  implicit none ; public
  type :: tracer_type
    real, dimension(:,:,:), pointer :: t => NULL()
    real :: conc_underflow = 0.0
    integer :: id_dfxy_conc = -1, id_dfxy_cont = -1, id_dfxy_cont_2d = -1, id_dfx_2d = -1, id_dfy_2d = -1
  end type tracer_type
  type :: tracer_registry_type
    integer :: ntr = 0
    type(tracer_type), allocatable :: Tr(:)
  end type tracer_registry_type
end module MOM_tracer_registry

module MOM_hor_bnd_diffusion
  use MOM_error_handler, only : standin_never
  implicit none ; public
  integer, parameter :: SURFACE = 1, BOTTOM = 2      ! (two distinct values: the stand-in tells nothing by them)
contains
  !> Never reached: only NDIFF_INTERIOR_ONLY and NDIFF_TAPERING, which the device refuses, look for the boundary layer's layers.
  subroutine boundary_k_range(boundary, nk, h, hbl, k_top, zeta_top, k_bot, zeta_bot)
    integer, intent(in) :: boundary, nk ; real, dimension(nk), intent(in) :: h ; real, intent(in) :: hbl
    integer, intent(out) :: k_top, k_bot ; real, intent(out) :: zeta_top, zeta_bot
    k_top = 1 ; k_bot = 1 ; zeta_top = 0.0 ; zeta_bot = 0.0
    call standin_never("boundary_k_range")
  end subroutine boundary_k_range
end module MOM_hor_bnd_diffusion

!> Types and constants only: the device refuses open boundaries and the doors leave the OBC pointer null, so that no member is
!! ever read.  The module has no procedure.
module MOM_open_boundary
  implicit none ; public
  integer, parameter :: OBC_NONE = 0, OBC_DIRECTION_N = 100, OBC_DIRECTION_S = 200, OBC_DIRECTION_E = 300, OBC_DIRECTION_W = 400
  type :: OBC_segment_type ; logical :: open = .false. ; end type OBC_segment_type
  type :: ocean_OBC_type
    logical :: open_u_BCs_exist_globally = .false., open_v_BCs_exist_globally = .false.
    logical :: u_E_OBCs_on_PE = .false., u_W_OBCs_on_PE = .false., v_N_OBCs_on_PE = .false., v_S_OBCs_on_PE = .false.
    integer :: Is_u_E_obc, Ie_u_E_obc, js_u_E_obc, je_u_E_obc, Is_u_W_obc, Ie_u_W_obc, js_u_W_obc, je_u_W_obc
    integer :: is_v_N_obc, ie_v_N_obc, Js_v_N_obc, Je_v_N_obc, is_v_S_obc, ie_v_S_obc, Js_v_S_obc, Je_v_S_obc
    integer, allocatable :: segnum_u(:,:), segnum_v(:,:)
    type(OBC_segment_type), allocatable :: segment(:)
  end type ocean_OBC_type
end module MOM_open_boundary

#elif !defined(STANDINS_AFTER_ENERGETIC_PBL)

module MOM_variables
  use MOM_EOS, only : EOS_type
  implicit none ; public
  type :: thermo_var_ptrs
    real, pointer, dimension(:,:,:) :: T => NULL(), S => NULL(), varT => NULL(), varS => NULL(), covarTS => NULL()
    real, pointer, dimension(:,:) :: p_surf => NULL()
    type(EOS_type), pointer :: eqn_of_state => NULL()
    real :: P_Ref = 0.0
    real, allocatable, dimension(:,:,:) :: SpV_avg
    integer :: valid_SpV_halo = -1
  end type thermo_var_ptrs
  type :: cont_diag_ptrs
    real, pointer, dimension(:,:,:) :: uhGM => NULL(), vhGM => NULL()
  end type cont_diag_ptrs
  type :: vertvisc_type
    real, allocatable, dimension(:,:) :: ustar_BBL, BBL_meanKE_loss, BBL_meanKE_loss_sqrtCd
    real, pointer, dimension(:,:) :: h_ML => NULL()
  end type vertvisc_type
end module MOM_variables

!> calc_resoln_function's wave speeds: not compared (the device has no calc_resoln_function), so both procedures count as FATAL.
!! VarMix_init calls wave_speed_init only with a resolution function, MEKE, an EBT structure or the FGNV streamfunction.
module MOM_wave_speed
  use MOM_error_handler, only : standin_never
  use MOM_grid, only : ocean_grid_type
  use MOM_verticalGrid, only : verticalGrid_type
  use MOM_unit_scaling, only : unit_scale_type
  use MOM_variables, only : thermo_var_ptrs
  implicit none ; public
  type :: wave_speed_CS ; integer :: dummy = 0 ; end type wave_speed_CS
contains
  subroutine wave_speed(h, tv, G, GV, US, cg1, CS, halo_size, use_ebt_mode, mono_N2_column_fraction, mono_N2_depth, modal_structure)
    type(ocean_grid_type), intent(in) :: G ; type(verticalGrid_type), intent(in) :: GV ; type(unit_scale_type), intent(in) :: US
    real, dimension(G%isd:G%ied,G%jsd:G%jed,GV%ke), intent(in) :: h ; type(thermo_var_ptrs), intent(in) :: tv
    real, dimension(G%isd:G%ied,G%jsd:G%jed), intent(out) :: cg1 ; type(wave_speed_CS), intent(in) :: CS
    integer, optional, intent(in) :: halo_size ; logical, optional, intent(in) :: use_ebt_mode
    real, optional, intent(in) :: mono_N2_column_fraction, mono_N2_depth
    real, dimension(G%isd:G%ied,G%jsd:G%jed,GV%ke), optional, intent(out) :: modal_structure
    cg1(:,:) = 0.0 ; if (present(modal_structure)) modal_structure(:,:,:) = 0.0
    call standin_never("wave_speed")
  end subroutine wave_speed
  subroutine wave_speed_init(CS, GV, use_ebt_mode, mono_N2_column_fraction, mono_N2_depth, remap_answers_2018, remap_answer_date, &
                             better_speed_est, om4_remap_via_sub_cells, min_speed, wave_speed_tol, c1_thresh)
    type(wave_speed_CS), intent(inout) :: CS ; type(verticalGrid_type), intent(in) :: GV
    logical, optional, intent(in) :: use_ebt_mode, remap_answers_2018, better_speed_est, om4_remap_via_sub_cells
    real, optional, intent(in) :: mono_N2_column_fraction, mono_N2_depth, min_speed, wave_speed_tol, c1_thresh
    integer, optional, intent(in) :: remap_answer_date
    call standin_never("wave_speed_init")
  end subroutine wave_speed_init
end module MOM_wave_speed

module MOM_wave_interface
  use MOM_grid, only : ocean_grid_type
  use MOM_verticalGrid, only : verticalGrid_type
  use MOM_unit_scaling, only : unit_scale_type
  implicit none ; public
  type :: wave_parameters_CS ; integer :: dummy = 0 ; end type wave_parameters_CS
contains
  !> Never reached: the device refuses use_LT, and the doors leave Waves null.
  subroutine get_Langmuir_Number(LA, G, GV, US, HBL, ustar, i, j, dz, Waves, U_H, V_H, Override_MA)
    real, intent(out) :: LA ; type(ocean_grid_type), intent(in) :: G ; type(verticalGrid_type), intent(in) :: GV
    type(unit_scale_type), intent(in) :: US ; real, intent(in) :: HBL, ustar ; integer, intent(in) :: i, j
    real, dimension(GV%ke), intent(in) :: dz ; type(wave_parameters_CS), pointer :: Waves
    real, dimension(GV%ke), optional, intent(in) :: U_H, V_H ; logical, optional, intent(in) :: Override_MA
    LA = 0.0
  end subroutine get_Langmuir_Number
end module MOM_wave_interface

module MOM_CVMix_KPP
  use MOM_error_handler, only : standin_never
  use MOM_grid, only : ocean_grid_type
  use MOM_unit_scaling, only : unit_scale_type
  implicit none ; public
  type :: KPP_CS ; integer :: dummy = 0 ; end type KPP_CS
contains
  !> Never reached: MOM_neutral_diffusion imports the name and does not call it.
  subroutine KPP_get_BLD(CS, BLD, G, US, m_to_BLD_units)
    type(KPP_CS), pointer :: CS ; type(ocean_grid_type), intent(in) :: G ; type(unit_scale_type), intent(in) :: US
    real, dimension(G%isd:G%ied,G%jsd:G%jed), intent(inout) :: BLD ; real, optional, intent(in) :: m_to_BLD_units
    call standin_never("KPP_get_BLD")
  end subroutine KPP_get_BLD
end module MOM_CVMix_KPP

#else

module MOM_diabatic_driver
  use MOM_error_handler, only : standin_never
  use MOM_CVMix_KPP, only : KPP_CS
  use MOM_energetic_PBL, only : energetic_PBL_CS
  implicit none ; public
  type :: diabatic_CS ; integer :: dummy = 0 ; end type diabatic_CS
contains
  !> Never reached by a compared case: neutral_diffusion_init asks for the boundary-layer schemes only with NDIFF_INTERIOR_ONLY,
  !! which the device refuses.  Both pointers come back null.
  subroutine extract_diabatic_member(CS, KPP_CSp, energetic_PBL_CSp)
    type(diabatic_CS), target, intent(in) :: CS
    type(KPP_CS), optional, pointer :: KPP_CSp ; type(energetic_PBL_CS), optional, pointer :: energetic_PBL_CSp
    if (present(KPP_CSp)) KPP_CSp => NULL()
    if (present(energetic_PBL_CSp)) energetic_PBL_CSp => NULL()
    call standin_never("extract_diabatic_member")
  end subroutine extract_diabatic_member
end module MOM_diabatic_driver
#endif
