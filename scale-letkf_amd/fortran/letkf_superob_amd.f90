!===============================================================================
! letkf_superob_amd.f90 -- Fortran side of include/letkf_amd_superob.h: superob on the device.  The BIND(C) mirrors of
! letkf_superob_params and letkf_superob_out (fields in C order), the interfaces of the entries of libletkf_amd_superob.so, and
!   superob_amd          stands where the four stages of PROGRAM superob stood (scale/obs/superob.f90:254-948), between the
!                        host's read_obs + phys2ijk and its unit conversions + write of the supTT.dat records (:959-1003)
!   superob_methods_amd  the reference's hard-coded obmethod_* tables (:120-151), obmethod(nobtype, nid)
! slot_off, elem_uid and the four method tables are HOST arrays (c_loc of a TARGET); the rows and every output are DEVICE arrays.
! The call is asynchronous on the context's stream: letkf_ctx_synchronize before a download.
!===============================================================================
MODULE letkf_superob_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_SUPEROB_VERSION = 1
  INTEGER(c_int32_t), PARAMETER :: LETKF_SUPEROB_SURFACE_TYPES = 18304      ! report types 8, 9, 10, 11, 15 (:289-291)

  TYPE, BIND(C) :: letkf_superob_params
    INTEGER(c_int64_t) :: nobs
    TYPE(c_ptr)        :: elm, typ                                  ! dev int32 (nobs)
    TYPE(c_ptr)        :: lon, lat, lev, dat, err, ri, rj, rk       ! dev real64 (nobs)
    TYPE(c_ptr)        :: slot_off                                  ! HOST int64 (0:nslots)
    INTEGER(c_int32_t) :: nlon, nlat, nlevx, nslots, nbslot, nobtype, nid, surface_typ_mask
    TYPE(c_ptr)        :: elem_uid                                  ! HOST int32 (nid)
    TYPE(c_ptr)        :: method_g, method_v, method_t, method_h    ! HOST int32 (nobtype, nid)
  END TYPE letkf_superob_params

  TYPE, BIND(C) :: letkf_superob_out
    TYPE(c_ptr)        :: elm, typ, slot                            ! dev int32 (nobs)
    TYPE(c_ptr)        :: lon, lat, lev, dat, err, ri, rj, rk       ! dev real64 (nobs)
    TYPE(c_ptr)        :: i, j, k                                   ! dev int32 (nobs)
    TYPE(c_ptr)        :: nout                                      ! dev int64 (1)
    TYPE(c_ptr)        :: slot_off_out                              ! dev int64 (0:nslots), or c_null_ptr
    TYPE(c_ptr)        :: qc1                                       ! dev int32 (nobs), or c_null_ptr
    TYPE(c_ptr)        :: counts                                    ! dev int64 (7), or c_null_ptr
    TYPE(c_ptr)        :: obsnum                                    ! dev int64 (nobtype, nid, 4), or c_null_ptr
  END TYPE letkf_superob_out

  INTERFACE
    FUNCTION letkf_superob_dev(ctx, p, o) BIND(C, name='letkf_superob_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_superob_params, letkf_superob_out
      TYPE(c_ptr), VALUE :: ctx
      TYPE(letkf_superob_params), INTENT(IN) :: p
      TYPE(letkf_superob_out), INTENT(IN) :: o
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_superob_default_methods(nobtype, nid, method_g, method_v, method_t, method_h) &
        BIND(C, name='letkf_superob_default_methods') RESULT(rc)
      IMPORT :: c_int, c_int32_t
      INTEGER(c_int32_t), VALUE :: nobtype, nid
      INTEGER(c_int32_t), INTENT(OUT) :: method_g(*), method_v(*), method_t(*), method_h(*)
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_superob_slot_priority(nslots, nbslot, slot_priority) BIND(C, name='letkf_superob_slot_priority') RESULT(rc)
      IMPORT :: c_int, c_int32_t
      INTEGER(c_int32_t), VALUE :: nslots, nbslot
      INTEGER(c_int32_t), INTENT(OUT) :: slot_priority(*)
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  SUBROUTINE superob_amd(ctx, prm, out, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_superob_params), INTENT(IN) :: prm
    TYPE(letkf_superob_out), INTENT(IN) :: out
    INTEGER, INTENT(OUT) :: ierr
    ierr = letkf_superob_dev(ctx, prm, out)
  END SUBROUTINE superob_amd

  SUBROUTINE superob_methods_amd(nobtype, nid, obmethod_g, obmethod_v, obmethod_t, obmethod_h, ierr)
    INTEGER, INTENT(IN) :: nobtype, nid
    INTEGER(c_int32_t), INTENT(OUT) :: obmethod_g(nobtype, nid), obmethod_v(nobtype, nid), obmethod_t(nobtype, nid), &
                                       obmethod_h(nobtype, nid)
    INTEGER, INTENT(OUT) :: ierr
    ierr = letkf_superob_default_methods(INT(nobtype, c_int32_t), INT(nid, c_int32_t), obmethod_g, obmethod_v, obmethod_t, &
                                         obmethod_h)
  END SUBROUTINE superob_methods_amd

END MODULE letkf_superob_amd
