!===============================================================================
! letkf_interp_amd.f90 -- Fortran side of include/letkf_amd_interp.h: weight interpolation, letkf_core on every s-th
! column of a tile and the analysis at every point.  The BIND(C) mirror of letkf_interp_args (fields in C order), the
! interfaces of the two entries and das_letkf_interp_amd, the sibling of das_letkf_amd (letkf_tools_amd.f90) for a
! rectangular tile nx x ny x nlev with point p = i + nx*j + nx*ny*lev.
!===============================================================================
MODULE letkf_interp_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_INTERP_VERSION = 1

  TYPE, BIND(C) :: letkf_interp_args
    INTEGER(c_int32_t) :: nx, ny, nlev, stride_x, stride_y, reserved0
    INTEGER(c_int64_t) :: ws_bytes
    TYPE(c_ptr)        :: rig, rjg, rlev, rz
    TYPE(c_ptr)        :: nobs_coarse
  END TYPE letkf_interp_args

  INTERFACE
    FUNCTION letkf_interp_coarse_axis(n, stride, idx, count) BIND(C, name='letkf_interp_coarse_axis') RESULT(rc)
      IMPORT :: c_int, c_int32_t
      INTEGER(c_int32_t), VALUE :: n, stride
      INTEGER(c_int32_t), INTENT(OUT) :: idx(*)
      INTEGER(c_int32_t), INTENT(OUT) :: count
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_das_interp_dev(ctx, args, tables, interp) BIND(C, name='letkf_das_interp_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_das_args, letkf_search_tables, letkf_interp_args
      TYPE(c_ptr), VALUE :: ctx
      TYPE(letkf_das_args), INTENT(IN) :: args
      TYPE(letkf_search_tables), INTENT(IN) :: tables
      TYPE(letkf_interp_args), INTENT(IN) :: interp
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! The analysis of the tile by weight interpolation.  args: the switches, the observation table, beta, infl and the
  ! state (perturbations, mean, deterministic member) as letkf_das_columns_dev takes them, all DEVICE pointers; npts and
  ! the outputs the route does not have are set here.  rig / rjg [nx*ny], rlev / rz [nx*ny*nlev] DEVICE pointers.
  ! ws_bytes: the library's workspace of a slab of levels (0: its default); nobs_coarse: c_null_ptr or a DEVICE array
  ! of the coarse points' local observation counts.  ierr: the entry's return code.
  SUBROUTINE das_letkf_interp_amd(ctx, args, tables, nx, ny, nlev, stride_x, stride_y, rig, rjg, rlev, rz, ws_bytes, &
                                  nobs_coarse, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_das_args), INTENT(IN) :: args
    TYPE(letkf_search_tables), INTENT(IN) :: tables
    INTEGER, INTENT(IN) :: nx, ny, nlev, stride_x, stride_y
    TYPE(c_ptr), INTENT(IN) :: rig, rjg, rlev, rz
    INTEGER(c_int64_t), INTENT(IN) :: ws_bytes
    TYPE(c_ptr), INTENT(IN) :: nobs_coarse
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_das_args) :: a
    TYPE(letkf_interp_args) :: ia

    a = args
    a%npts = INT(nx, c_int64_t)*INT(ny, c_int64_t)*INT(nlev, c_int64_t)
    a%infl_adaptive = 0                   ! (the adaptive update belongs to solved points)
    a%obs_off = c_null_ptr; a%obs_idx = c_null_ptr; a%rdiag_l = c_null_ptr; a%rloc_l = c_null_ptr
    a%trans_out = c_null_ptr; a%transm_out = c_null_ptr; a%pa_out = c_null_ptr; a%nsweep = c_null_ptr
    ia%nx = nx; ia%ny = ny; ia%nlev = nlev; ia%stride_x = stride_x; ia%stride_y = stride_y; ia%reserved0 = 0
    ia%ws_bytes = ws_bytes
    ia%rig = rig; ia%rjg = rjg; ia%rlev = rlev; ia%rz = rz
    ia%nobs_coarse = nobs_coarse
    ierr = letkf_das_interp_dev(ctx, a, tables, ia)
  END SUBROUTINE das_letkf_interp_amd

END MODULE letkf_interp_amd
