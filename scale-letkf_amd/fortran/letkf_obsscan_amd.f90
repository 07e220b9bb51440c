!===============================================================================
! letkf_obsscan_amd.f90 -- Fortran side of include/letkf_amd_obsscan.h: obsope_cal's first scan on the device.  The BIND(C)
! mirrors of letkf_obsscan_params, letkf_obsscan_out and letkf_obsscan_lists (fields in C order), the interfaces of the entries
! of libletkf_amd_obsscan.so, and
!   obsscan_amd       stands where the first scan and the bucket sort of obsope_cal stood (scale/obs/obsope_tools.f90:140-427):
!                     obsda's set / idx / qc for every subdomain, bsn(SLOT_START:SLOT_END+2, 0:nprocs_d-1) and
!                     bsna(SLOT_START-1:SLOT_END+2, 0:nprocs_d-1) with the reference's bounds
!   obsope_slot_amd   stands where the loop over the rows of one time slot stood (:454-507), for subdomain ip
! off, obsda_run, bsn and bsna are HOST arrays; the rows, dif and the lists are DEVICE arrays.  obsscan_amd returns after its one
! read-back (the tables); the lists are then complete on the context's stream.
!===============================================================================
MODULE letkf_obsscan_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_obsope_amd
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_OBSSCAN_VERSION = 1

  TYPE, BIND(C) :: letkf_obsscan_params
    TYPE(c_ptr)        :: dif                                       ! dev real64, per file row
    TYPE(c_ptr)        :: obsda_run                                 ! HOST int32 (nfile), or c_null_ptr: every file runs
    INTEGER(c_int32_t) :: nlon, nlat, ihalo, jhalo, prc_num_x, prc_num_y
    INTEGER(c_int32_t) :: slot_start, slot_end, slot_base, myrank_d
    REAL(c_double)     :: slot_tinterval
  END TYPE letkf_obsscan_params

  TYPE, BIND(C) :: letkf_obsscan_out
    TYPE(c_ptr)        :: set, idx, qc                              ! dev int32 (rows of the obsda_run files)
    TYPE(c_ptr)        :: bsn                                       ! HOST int32 (nslots+2, nprocs_d)
    TYPE(c_ptr)        :: bsna                                      ! HOST int32 (nslots+3, nprocs_d)
    TYPE(c_ptr)        :: rank, slot, own                           ! dev int32 (file rows), or c_null_ptr
  END TYPE letkf_obsscan_out

  TYPE, BIND(C) :: letkf_obsscan_lists
    INTEGER(c_int32_t) :: nprocs_d, slot_start, slot_end, reserved0
    TYPE(c_ptr)        :: bsna                                      ! HOST int32 (nslots+3, nprocs_d)
    TYPE(c_ptr)        :: set, idx                                  ! dev int32, the global lists
    TYPE(c_ptr)        :: qc                                        ! dev int32, INOUT
  END TYPE letkf_obsscan_lists

  INTERFACE
    FUNCTION letkf_obsscan_dev(ctx, p, files, o) BIND(C, name='letkf_obsscan_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_obsscan_params, letkf_obs_file_rows, letkf_obsscan_out
      TYPE(c_ptr), VALUE :: ctx
      TYPE(letkf_obsscan_params), INTENT(IN) :: p
      TYPE(letkf_obs_file_rows), INTENT(IN) :: files
      TYPE(letkf_obsscan_out), INTENT(IN) :: o
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obsscan_rows(bsna, nprocs_d, slot_start, slot_end, ip, islot, first, count) &
        BIND(C, name='letkf_obsscan_rows') RESULT(rc)
      IMPORT :: c_int, c_int32_t, c_int64_t
      INTEGER(c_int32_t), INTENT(IN) :: bsna(*)
      INTEGER(c_int32_t), VALUE :: nprocs_d, slot_start, slot_end, ip, islot
      INTEGER(c_int64_t), INTENT(OUT) :: first, count
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obsscan_slot_bounds(slot_start, slot_end, slot_base, slot_tinterval, slot_lb, slot_ub) &
        BIND(C, name='letkf_obsscan_slot_bounds') RESULT(rc)
      IMPORT :: c_int, c_int32_t, c_double
      INTEGER(c_int32_t), VALUE :: slot_start, slot_end, slot_base
      REAL(c_double), VALUE :: slot_tinterval
      REAL(c_double), INTENT(OUT) :: slot_lb(*), slot_ub(*)
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obsope_slot_dev(ctx, l, ip, islot, p, files, f, ensval, kld) BIND(C, name='letkf_obsope_slot_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t, letkf_obsscan_lists, letkf_obsope_params, letkf_obs_file_rows, letkf_obsope_fields
      TYPE(c_ptr), VALUE :: ctx, ensval
      TYPE(letkf_obsscan_lists), INTENT(IN) :: l
      INTEGER(c_int32_t), VALUE :: ip, islot
      TYPE(letkf_obsope_params), INTENT(IN) :: p
      TYPE(letkf_obs_file_rows), INTENT(IN) :: files
      TYPE(letkf_obsope_fields), INTENT(IN) :: f
      INTEGER(c_int64_t), VALUE :: kld
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! The first scan over the rows of nfile files: off (HOST, 0-based offsets), ri, rj, dif (DEVICE, per file row); prm: the
  ! layout, the slots and obsda_run (prm%dif is set here).  set, idx, qc: DEVICE, one entry per row of the files that run.
  SUBROUTINE obsscan_amd(ctx, prm, nfile, off, ri, rj, dif, set, idx, qc, bsn, bsna, ierr, rank)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_obsscan_params), INTENT(IN) :: prm
    INTEGER, INTENT(IN) :: nfile
    INTEGER(c_int64_t), INTENT(IN), TARGET :: off(nfile + 1)
    TYPE(c_ptr), INTENT(IN) :: ri, rj, dif, set, idx, qc
    INTEGER(c_int32_t), INTENT(OUT), TARGET :: bsn(prm%slot_start:prm%slot_end + 2, 0:prm%prc_num_x*prm%prc_num_y - 1)
    INTEGER(c_int32_t), INTENT(OUT), TARGET :: bsna(prm%slot_start - 1:prm%slot_end + 2, 0:prm%prc_num_x*prm%prc_num_y - 1)
    INTEGER, INTENT(OUT) :: ierr
    TYPE(c_ptr), INTENT(IN), OPTIONAL :: rank                        ! DEVICE int32 per file row: obs%rank
    TYPE(letkf_obs_file_rows) :: files
    TYPE(letkf_obsscan_params) :: p
    TYPE(letkf_obsscan_out) :: o

    files%nfile = nfile; files%reserved0 = 0
    files%off = c_loc(off)
    files%elm = c_null_ptr; files%typ = c_null_ptr; files%lev = c_null_ptr     ! (the scan reads ri and rj only)
    files%dat = c_null_ptr; files%err = c_null_ptr
    files%ri = ri; files%rj = rj
    p = prm; p%dif = dif
    o%set = set; o%idx = idx; o%qc = qc; o%bsn = c_loc(bsn); o%bsna = c_loc(bsna)
    o%rank = c_null_ptr; o%slot = c_null_ptr; o%own = c_null_ptr
    IF (PRESENT(rank)) o%rank = rank
    ierr = letkf_obsscan_dev(ctx, p, files, o)
  END SUBROUTINE obsscan_amd

  ! H(x) of fields%nmem members for the list rows of subdomain ip (0-based, as myrank_d) in slot islot; files as obsope_amd
  ! takes them; ensval (DEVICE) is indexed by the global list row.
  SUBROUTINE obsope_slot_amd(ctx, lists, ip, islot, prm, nfile, off, elm, typ, lev, ri, rj, fields, ensval, kld, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_obsscan_lists), INTENT(IN) :: lists
    INTEGER, INTENT(IN) :: ip, islot
    TYPE(letkf_obsope_params), INTENT(IN) :: prm
    INTEGER, INTENT(IN) :: nfile
    INTEGER(c_int64_t), INTENT(IN), TARGET :: off(nfile + 1)
    TYPE(c_ptr), INTENT(IN) :: elm, typ, lev, ri, rj
    TYPE(letkf_obsope_fields), INTENT(IN) :: fields
    TYPE(c_ptr), INTENT(IN) :: ensval
    INTEGER(c_int64_t), INTENT(IN) :: kld
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_obs_file_rows) :: files

    files%nfile = nfile; files%reserved0 = 0
    files%off = c_loc(off)
    files%elm = elm; files%typ = typ; files%lev = lev; files%ri = ri; files%rj = rj
    files%dat = c_null_ptr; files%err = c_null_ptr
    ierr = letkf_obsope_slot_dev(ctx, lists, INT(ip, c_int32_t), INT(islot, c_int32_t), prm, files, fields, ensval, kld)
  END SUBROUTINE obsope_slot_amd

END MODULE letkf_obsscan_amd
