!===============================================================================
! letkf_obsmake_amd.f90 -- Fortran side of include/letkf_amd_obsmake.h: obsmake_cal on the device.  The BIND(C) mirrors of
! letkf_obsmake_slot and letkf_obsmake_err (fields in C order), the interfaces of the entries of libletkf_amd_osse.so, and
!   rand_create_amd      init_gen_rand(seed) of a fresh process (the clock seed idate(8) + idate(7)*1000 is the caller's)
!   obsmake_slot_amd     stands where the loop over the rows of one time slot stood (obsope_tools.f90:819-982)
!   obsmake_noise_amd    stands where com_randn and the loop at :1006-1049 stood, after the MPI_REDUCE of dat
! Zeroing dat before the first slot, the MPI_REDUCE, write_obs_all and reading the nature run stay the host's.
!===============================================================================
MODULE letkf_obsmake_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_obsope_amd
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_OBSMAKE_VERSION = 1

  TYPE, BIND(C) :: letkf_obsmake_slot
    REAL(c_double)     :: slot_lb, slot_ub
    TYPE(c_ptr)        :: dif                         ! dev, per file row
    TYPE(c_ptr)        :: own                         ! dev int32 per file row, or c_null_ptr (all 1)
    INTEGER(c_int32_t) :: outside_undef
    INTEGER(c_int32_t) :: reserved0
  END TYPE letkf_obsmake_slot

  TYPE, BIND(C) :: letkf_obsmake_err
    REAL(c_double)     :: obserr_u, obserr_v, obserr_t, obserr_q, obserr_rh, obserr_ps, obserr_radar_ref, obserr_radar_vr
  END TYPE letkf_obsmake_err

  INTERFACE
    FUNCTION letkf_rand_create(seed, r) BIND(C, name='letkf_rand_create') RESULT(rc)
      IMPORT :: c_int, c_int32_t, c_ptr
      INTEGER(c_int32_t), VALUE :: seed
      TYPE(c_ptr), INTENT(OUT) :: r
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_rand_destroy(r) BIND(C, name='letkf_rand_destroy') RESULT(rc)
      IMPORT :: c_int, c_ptr
      TYPE(c_ptr), VALUE :: r
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_rand_set_chunk(r, pairs) BIND(C, name='letkf_rand_set_chunk') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t
      TYPE(c_ptr), VALUE :: r
      INTEGER(c_int64_t), VALUE :: pairs
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_rand_res53(r, n, out) BIND(C, name='letkf_rand_res53') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t
      TYPE(c_ptr), VALUE :: r, out
      INTEGER(c_int64_t), VALUE :: n
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_randn_dev(ctx, r, n, out) BIND(C, name='letkf_randn_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t
      TYPE(c_ptr), VALUE :: ctx, r, out
      INTEGER(c_int64_t), VALUE :: n
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obsmake_slot_dev(ctx, s, op, files, f, counts) BIND(C, name='letkf_obsmake_slot_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_obsmake_slot, letkf_obsope_params, letkf_obs_file_rows, letkf_obsope_fields
      TYPE(c_ptr), VALUE :: ctx, counts
      TYPE(letkf_obsmake_slot), INTENT(IN) :: s
      TYPE(letkf_obsope_params), INTENT(IN) :: op
      TYPE(letkf_obs_file_rows), INTENT(IN) :: files
      TYPE(letkf_obsope_fields), INTENT(IN) :: f
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obsmake_noise_dev(ctx, e, files, r) BIND(C, name='letkf_obsmake_noise_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_obsmake_err, letkf_obs_file_rows
      TYPE(c_ptr), VALUE :: ctx, r
      TYPE(letkf_obsmake_err), INTENT(IN) :: e
      TYPE(letkf_obs_file_rows), INTENT(IN) :: files
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! The stream of a process's first init_gen_rand(seed).  obsmake's own seed is the clock's, idate(8) + idate(7)*1000 from
  ! DATE_AND_TIME (common.f90:272-274): pass that to reproduce its habit, or a fixed seed to reproduce an OSSE.
  SUBROUTINE rand_create_amd(seed, rand, ierr)
    INTEGER, INTENT(IN) :: seed
    TYPE(c_ptr), INTENT(OUT) :: rand
    INTEGER, INTENT(OUT) :: ierr
    ierr = letkf_rand_create(INT(seed, c_int32_t), rand)
  END SUBROUTINE rand_create_amd

  ! One time slot: dat (DEVICE) of the rows with slot%slot_lb < dif <= slot%slot_ub becomes H(x) of the one state in
  ! `fields`, or undef.  nfile, off (HOST), elm .. rj, dat (DEVICE): the observation files; counts: DEVICE int64 (2) or
  ! c_null_ptr -- nslot and nobs_slot.  prm%rotc, where given, is per FILE row.
  SUBROUTINE obsmake_slot_amd(ctx, slot, prm, nfile, off, elm, typ, lev, ri, rj, dat, fields, counts, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_obsmake_slot), INTENT(IN) :: slot
    TYPE(letkf_obsope_params), INTENT(IN) :: prm
    INTEGER, INTENT(IN) :: nfile
    INTEGER(c_int64_t), INTENT(IN), TARGET :: off(nfile + 1)
    TYPE(c_ptr), INTENT(IN) :: elm, typ, lev, ri, rj, dat
    TYPE(letkf_obsope_fields), INTENT(IN) :: fields
    TYPE(c_ptr), INTENT(IN) :: counts
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_obs_file_rows) :: files

    files%nfile = nfile; files%reserved0 = 0
    files%off = c_loc(off)
    files%elm = elm; files%typ = typ; files%lev = lev; files%ri = ri; files%rj = rj
    files%dat = dat; files%err = c_null_ptr
    ierr = letkf_obsmake_slot_dev(ctx, slot, prm, files, fields, counts)
  END SUBROUTINE obsmake_slot_amd

  ! err by element and dat = dat + err * com_randn over all rows of all files in file order (elm, dat, err: DEVICE)
  SUBROUTINE obsmake_noise_amd(ctx, errs, nfile, off, elm, dat, err, rand, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_obsmake_err), INTENT(IN) :: errs
    INTEGER, INTENT(IN) :: nfile
    INTEGER(c_int64_t), INTENT(IN), TARGET :: off(nfile + 1)
    TYPE(c_ptr), INTENT(IN) :: elm, dat, err, rand
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_obs_file_rows) :: files

    files%nfile = nfile; files%reserved0 = 0
    files%off = c_loc(off)
    files%elm = elm; files%typ = c_null_ptr; files%lev = c_null_ptr; files%ri = c_null_ptr; files%rj = c_null_ptr
    files%dat = dat; files%err = err
    ierr = letkf_obsmake_noise_dev(ctx, errs, files, rand)
  END SUBROUTINE obsmake_noise_amd

END MODULE letkf_obsmake_amd
