!===============================================================================
! letkf_obsope_amd.f90 -- Fortran side of include/letkf_amd_obsope.h: the observation operator of obsope_cal on the
! device.  The BIND(C) mirrors of letkf_obsope_fields and letkf_obsope_params (fields in C order), the interface of the
! entry and obsope_amd, the call that stands where obsope_cal's loop over the rows of a time slot stood.
!===============================================================================
MODULE letkf_obsope_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_OBSOPE_VERSION = 1

  TYPE, BIND(C) :: letkf_obsope_fields
    INTEGER(c_int32_t) :: nlev, nlon, nlat, khalo, ihalo, jhalo
    INTEGER(c_int32_t) :: nv3dd, nv2dd
    INTEGER(c_int32_t) :: nmem, m0
    TYPE(c_ptr)        :: v3d
    INTEGER(c_int64_t) :: s3k, s3i, s3j, s3v, s3m
    TYPE(c_ptr)        :: v2d
    INTEGER(c_int64_t) :: s2i, s2j, s2v, s2m
  END TYPE letkf_obsope_fields

  TYPE, BIND(C) :: letkf_obsope_params
    TYPE(c_ptr)        :: lon, lat                    ! dev, per file row
    TYPE(c_ptr)        :: file_radar                  ! HOST int32 [nfile]
    TYPE(c_ptr)        :: radar_meta                  ! HOST real64 [nradar][3]
    TYPE(c_ptr)        :: rotc                        ! dev [rows][2] or c_null_ptr
    TYPE(c_ptr)        :: use_obs                     ! HOST int32 [nobtype]
    INTEGER(c_int32_t) :: nobtype, method_ref_calc, use_terminal_velocity, stggrd
    REAL(c_double)     :: min_radar_ref_dbz, low_ref_shift, radar_zmax, ps_adjust_thres, ri_off, rj_off
  END TYPE letkf_obsope_params

  INTERFACE
    FUNCTION letkf_obsope_dev(ctx, p, files, f, row0, nrows, set, idx, qc, ensval, kld) &
        BIND(C, name='letkf_obsope_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t, letkf_obsope_params, letkf_obs_file_rows, letkf_obsope_fields
      TYPE(c_ptr), VALUE :: ctx, set, idx, qc, ensval
      TYPE(letkf_obsope_params), INTENT(IN) :: p
      TYPE(letkf_obs_file_rows), INTENT(IN) :: files
      TYPE(letkf_obsope_fields), INTENT(IN) :: f
      INTEGER(c_int64_t), VALUE :: row0, nrows, kld
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! H(x) of fields%nmem members for the obsda rows n1 .. n2 (1-based, as obsope_cal's loop bounds) into
  ! ensval(fields%m0 + 1 .. fields%m0 + nmem, n), qc merged by maximum.  prm: the switches and the per-row arrays the
  ! operator needs beyond the files; nfile, off (HOST), elm .. rj (DEVICE): the observation files as set_letkf_obs_amd takes
  ! them, BEFORE that call pre-processes them.  set, idx, qc, ensval: DEVICE pointers of obsda; kld: doubles per ensval row.
  SUBROUTINE obsope_amd(ctx, prm, nfile, off, elm, typ, lev, ri, rj, fields, n1, n2, set, idx, qc, ensval, kld, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_obsope_params), INTENT(IN) :: prm
    INTEGER, INTENT(IN) :: nfile
    INTEGER(c_int64_t), INTENT(IN), TARGET :: off(nfile + 1)
    TYPE(c_ptr), INTENT(IN) :: elm, typ, lev, ri, rj
    TYPE(letkf_obsope_fields), INTENT(IN) :: fields
    INTEGER(c_int64_t), INTENT(IN) :: n1, n2
    TYPE(c_ptr), INTENT(IN) :: set, idx, qc, ensval
    INTEGER(c_int64_t), INTENT(IN) :: kld
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_obs_file_rows) :: files

    files%nfile = nfile; files%reserved0 = 0
    files%off = c_loc(off)
    files%elm = elm; files%typ = typ; files%lev = lev; files%ri = ri; files%rj = rj
    files%dat = c_null_ptr; files%err = c_null_ptr                       ! (the operator does not read them)
    ierr = letkf_obsope_dev(ctx, prm, files, fields, n1 - 1, n2 - n1 + 1, set, idx, qc, ensval, kld)
  END SUBROUTINE obsope_amd

END MODULE letkf_obsope_amd
