!===============================================================================
! letkf_nobsout_amd.f90 -- Fortran side of include/letkf_amd_nobsout.h: NOBS_OUT on the device.  The BIND(C) mirror of
! letkf_nobsout_params (fields in C order), the interfaces of the two entries of libletkf_amd_nobsout.so, and
!   nobs_fields_amd   stands where work3dn is filled (scale/letkf/letkf_tools.f90:440-447) and the eleven fields are picked from it
!                     (:768-778), for one variable class; the reference's uids, radar type and picks are the defaults
! letkf_das_columns_nobs_dev takes the arguments of letkf_das_columns_dev and two more device arrays, (nctype, nij1*nlev) in
! Fortran order: it replaces that call where NOBS_OUT is set (INTEGRATION.md, level 2).
! elm_u_ctype and typ_ctype are HOST arrays, as letkf_obs_table_info_get returns them; everything else is a DEVICE array.
!===============================================================================
MODULE letkf_nobsout_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_NOBSOUT_VERSION = 1
  INTEGER, PARAMETER :: LETKF_NOBSOUT_NFIELDS = 11

  TYPE, BIND(C) :: letkf_nobsout_params
    INTEGER(c_int32_t) :: nctype, nobtype
    INTEGER(c_int32_t) :: uid_ref, uid_re0, uid_vr, typ_radar
    INTEGER(c_int32_t) :: pick(5)
    INTEGER(c_int32_t) :: reserved0
    TYPE(c_ptr)        :: elm_u_ctype                               ! HOST int32 (nctype)
    TYPE(c_ptr)        :: typ_ctype                                 ! HOST int32 (nctype)
  END TYPE letkf_nobsout_params

  INTERFACE
    FUNCTION letkf_das_columns_nobs_dev(ctx, args, tables, nij1, nlev, rig, rjg, rlev, rz, list_bytes, nobs_out, nobs_ctype, &
                                        cutd_ctype) BIND(C, name='letkf_das_columns_nobs_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t, letkf_das_args, letkf_search_tables
      TYPE(c_ptr), VALUE :: ctx, rig, rjg, rlev, rz, nobs_out, nobs_ctype, cutd_ctype
      TYPE(letkf_das_args), INTENT(IN) :: args
      TYPE(letkf_search_tables), INTENT(IN) :: tables
      INTEGER(c_int64_t), VALUE :: nij1, list_bytes
      INTEGER(c_int32_t), VALUE :: nlev
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_nobs_fields_dev(ctx, p, npts, nobs_ctype, cutd_ctype, work3dn, fields, sp, sv) &
        BIND(C, name='letkf_nobs_fields_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t, letkf_nobsout_params
      TYPE(c_ptr), VALUE :: ctx, nobs_ctype, cutd_ctype, work3dn, fields
      TYPE(letkf_nobsout_params), INTENT(IN) :: p
      INTEGER(c_int64_t), VALUE :: npts, sp, sv
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! work3dn (nobtype+6, npts) and / or work3d (npts, 11) on the device from nobs_ctype / cutd_ctype (nctype, npts) of
  ! letkf_das_columns_nobs_dev; c_null_ptr for an output that is not wanted, or for cutd_ctype (zeros in the cut-off rows)
  SUBROUTINE nobs_fields_amd(ctx, nctype, elm_u_ctype, typ_ctype, nobtype, npts, nobs_ctype, cutd_ctype, work3dn, work3d, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    INTEGER, INTENT(IN) :: nctype, nobtype
    INTEGER(c_int32_t), INTENT(IN), TARGET :: elm_u_ctype(nctype), typ_ctype(nctype)
    INTEGER(c_int64_t), INTENT(IN) :: npts
    TYPE(c_ptr), INTENT(IN) :: nobs_ctype, cutd_ctype, work3dn, work3d
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_nobsout_params) :: p

    p%nctype = nctype; p%nobtype = nobtype
    p%uid_ref = 9; p%uid_re0 = 10; p%uid_vr = 11; p%typ_radar = 22          ! :442-447
    p%pick = (/1, 3, 4, 8, 22/)                                             ! :768-772
    p%reserved0 = 0
    p%elm_u_ctype = c_loc(elm_u_ctype); p%typ_ctype = c_loc(typ_ctype)
    ierr = letkf_nobs_fields_dev(ctx, p, npts, nobs_ctype, cutd_ctype, work3dn, work3d, 1_c_int64_t, npts)
  END SUBROUTINE nobs_fields_amd

END MODULE letkf_nobsout_amd
