!===============================================================================
! letkf_interp_window_amd.f90 -- Fortran side of include/letkf_amd_interp_window.h: weight interpolation on a tile of a
! larger domain, with the coarse lattice of the whole domain.  The BIND(C) mirror of letkf_interp_window (fields in C
! order), the interfaces of the two entries and das_letkf_interp_window_amd, the sibling of das_letkf_interp_amd
! (letkf_interp_amd.f90) for arrays of nx x ny x nlev points that hold the owned rectangle and its halo.
!===============================================================================
MODULE letkf_interp_window_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_interp_amd
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_INTERP_WINDOW_VERSION = 1

  TYPE, BIND(C) :: letkf_interp_window
    INTEGER(c_int32_t) :: gnx, gny
    INTEGER(c_int32_t) :: gi0, gj0
    INTEGER(c_int32_t) :: oi0, oj0
    INTEGER(c_int32_t) :: onx, ony
  END TYPE letkf_interp_window

  INTERFACE
    FUNCTION letkf_interp_window_axis(gn, stride, g0, n, o0, on, idx, count) BIND(C, name='letkf_interp_window_axis') RESULT(rc)
      IMPORT :: c_int, c_int32_t
      INTEGER(c_int32_t), VALUE :: gn, stride, g0, n, o0, on
      INTEGER(c_int32_t), INTENT(OUT) :: idx(*)
      INTEGER(c_int32_t), INTENT(OUT) :: count
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_das_interp_window_dev(ctx, args, tables, interp, window) BIND(C, name='letkf_das_interp_window_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_das_args, letkf_search_tables, letkf_interp_args, letkf_interp_window
      TYPE(c_ptr), VALUE :: ctx
      TYPE(letkf_das_args), INTENT(IN) :: args
      TYPE(letkf_search_tables), INTENT(IN) :: tables
      TYPE(letkf_interp_args), INTENT(IN) :: interp
      TYPE(letkf_interp_window), INTENT(IN) :: window
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! The analysis of the owned rectangle by weight interpolation on the domain's lattice.  Arguments as das_letkf_interp_amd,
  ! nx / ny / nlev being the extents of the arrays; then the window, all 0-BASED as in the header: gnx, gny the domain,
  ! gi0, gj0 the global index of the arrays' first column, oi0, oj0 the first owned column in array indices, onx, ony the
  ! owned extent.  Of the halo only the coarse columns letkf_interp_window_axis names need to hold data.
  SUBROUTINE das_letkf_interp_window_amd(ctx, args, tables, nx, ny, nlev, stride_x, stride_y, rig, rjg, rlev, rz, ws_bytes, &
                                         nobs_coarse, gnx, gny, gi0, gj0, oi0, oj0, onx, ony, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_das_args), INTENT(IN) :: args
    TYPE(letkf_search_tables), INTENT(IN) :: tables
    INTEGER, INTENT(IN) :: nx, ny, nlev, stride_x, stride_y
    TYPE(c_ptr), INTENT(IN) :: rig, rjg, rlev, rz
    INTEGER(c_int64_t), INTENT(IN) :: ws_bytes
    TYPE(c_ptr), INTENT(IN) :: nobs_coarse
    INTEGER, INTENT(IN) :: gnx, gny, gi0, gj0, oi0, oj0, onx, ony
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_das_args) :: a
    TYPE(letkf_interp_args) :: ia
    TYPE(letkf_interp_window) :: w

    a = args
    a%npts = INT(nx, c_int64_t)*INT(ny, c_int64_t)*INT(nlev, c_int64_t)
    a%infl_adaptive = 0                   ! (the adaptive update belongs to solved points)
    a%obs_off = c_null_ptr; a%obs_idx = c_null_ptr; a%rdiag_l = c_null_ptr; a%rloc_l = c_null_ptr
    a%trans_out = c_null_ptr; a%transm_out = c_null_ptr; a%pa_out = c_null_ptr; a%nsweep = c_null_ptr
    ia%nx = nx; ia%ny = ny; ia%nlev = nlev; ia%stride_x = stride_x; ia%stride_y = stride_y; ia%reserved0 = 0
    ia%ws_bytes = ws_bytes
    ia%rig = rig; ia%rjg = rjg; ia%rlev = rlev; ia%rz = rz
    ia%nobs_coarse = nobs_coarse
    w%gnx = gnx; w%gny = gny; w%gi0 = gi0; w%gj0 = gj0; w%oi0 = oi0; w%oj0 = oj0; w%onx = onx; w%ony = ony
    ierr = letkf_das_interp_window_dev(ctx, a, tables, ia, w)
  END SUBROUTINE das_letkf_interp_window_amd

END MODULE letkf_interp_window_amd
