!===============================================================================
! letkf_obssim_amd.f90 -- Fortran side of include/letkf_amd_obssim.h: obssim_cal on the device.  The BIND(C) mirrors of
! letkf_obssim_params and letkf_obssim_out (fields in C order), the interface of the entry of libletkf_amd_obssim.so, and
!   obssim_cal_amd       stands where CALL obssim_cal(v3dgh, v2dgh, v3dgsim, v2dgsim, stggrd) stood (obssim.f90:86, :99), with the
!                        history fields on the device (`fields`; from state_to_history_amd in the `restart` branch) and the
!                        records of write_grd_mpi as a third output
! The host supplies in prm what obssim_cal takes from modules: the lists and the radar of the namelist (OBSSIM_*), lon / lat
! (MPRJ_xy2lonlat * rad2deg per interior column) and rotc (MPRJ_rotcoef).  stggrd is explicit: 1 in the `restart` branch, 0 in
! the `history` branch (the reference's `INTEGER :: stggrd_ = 0` is SAVEd and never reset by a call without the argument).
! Reading the files, the projection, the MPI_REDUCE into the global record and the file stay the host's.
!===============================================================================
MODULE letkf_obssim_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_obsope_amd
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_OBSSIM_VERSION = 1
  INTEGER, PARAMETER :: LETKF_OBSSIM_MAX_VARS = 16

  TYPE, BIND(C) :: letkf_obssim_params
    INTEGER(c_int32_t) :: nvar3, vars3(16)            ! OBSSIM_NUM_3D_VARS, OBSSIM_3D_VARS_LIST
    INTEGER(c_int32_t) :: nvar2, vars2(16)            ! OBSSIM_NUM_2D_VARS, OBSSIM_2D_VARS_LIST
    REAL(c_double)     :: radar_lon, radar_lat, radar_z
    TYPE(c_ptr)        :: lon, lat                    ! dev (nlon, nlat), degrees
    TYPE(c_ptr)        :: rotc                        ! dev (2, nlon, nlat), or c_null_ptr
    INTEGER(c_int32_t) :: method_ref_calc, use_terminal_velocity, stggrd, round_single
    REAL(c_double)     :: min_radar_ref_dbz, low_ref_shift, ps_adjust_thres
  END TYPE letkf_obssim_params

  TYPE, BIND(C) :: letkf_obssim_out
    TYPE(c_ptr)        :: v3, v2                      ! dev real64 (nlev, nlon, nlat, nvar3) / (nlon, nlat, nvar2), or c_null_ptr
    TYPE(c_ptr)        :: rec                         ! dev real32 (nlon, nlat, nrec, nstate), or c_null_ptr
    INTEGER(c_int64_t) :: sm3, sm2
  END TYPE letkf_obssim_out

  INTERFACE
    FUNCTION letkf_obssim_dev(ctx, p, f, o) BIND(C, name='letkf_obssim_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_obssim_params, letkf_obsope_fields, letkf_obssim_out
      TYPE(c_ptr), VALUE :: ctx
      TYPE(letkf_obssim_params), INTENT(IN) :: p
      TYPE(letkf_obsope_fields), INTENT(IN) :: f
      TYPE(letkf_obssim_out), INTENT(IN) :: o
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! v3dgsim, v2dgsim, rec: DEVICE arrays or c_null_ptr (not all three); fields%nmem states, dense one after the other.
  SUBROUTINE obssim_cal_amd(ctx, fields, v3dgsim, v2dgsim, stggrd, prm, rec, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_obsope_fields), INTENT(IN) :: fields
    TYPE(c_ptr), INTENT(IN) :: v3dgsim, v2dgsim, rec
    INTEGER, INTENT(IN) :: stggrd
    TYPE(letkf_obssim_params), INTENT(IN) :: prm
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_obssim_params) :: p
    TYPE(letkf_obssim_out) :: o

    p = prm
    p%stggrd = stggrd
    o%v3 = v3dgsim; o%v2 = v2dgsim; o%rec = rec
    o%sm3 = INT(fields%nlev, c_int64_t)*fields%nlon*fields%nlat*prm%nvar3
    o%sm2 = INT(fields%nlon, c_int64_t)*fields%nlat*prm%nvar2
    ierr = letkf_obssim_dev(ctx, p, fields, o)
  END SUBROUTINE obssim_cal_amd

END MODULE letkf_obssim_amd
