!===============================================================================
! obsfile_driver.f90 -- the independent check of the record framing: Fortran's own sequential unformatted I/O on one side, the
! device codec of include/letkf_amd_obsfile.h on the other.
!   1. WRITE(iunit) wk into conventional, radar and obsda files (FORM='unformatted', ACCESS='sequential'), read their bytes with
!      ACCESS='stream', decode / assemble on the device, compare with what was written (read_obs' SELECT CASE applied here in
!      REAL(4), as the reference applies it)
!   2. encode on the device, write the bytes with ACCESS='stream', read them back with sequential READ(iunit) wk, compare
! Prints one PASS / FAIL line per check; tests/test_fortran_obsfile.py reads them.  Argument: a directory to write into.
!===============================================================================
PROGRAM obsfile_driver
  USE letkf_obsfile_amd
  IMPLICIT NONE
  INTEGER, PARAMETER :: n = 300, nmem = 3, r_sngl = c_float, r_size = c_double
  INTEGER, PARAMETER :: ids(9) = (/2819, 2820, 3073, 3074, 3330, 3331, 14593, 99993, 4001/)
  REAL(r_sngl) :: wk(8), wd(4), tmp
  REAL(r_sngl) :: fil(8, n), rad(7, n), da(4, n, nmem)
  INTEGER(c_int32_t), TARGET :: elm(n), typ(n), set(n), idx(n), qc(n), col(nmem)
  REAL(r_size), TARGET :: lon(n), lat(n), lev(n), dat(n), err(n), dif(n), ensval(nmem, n), meta(3)
  INTEGER(c_int32_t) :: x_elm(n), x_typ(n), x_qc(n)
  REAL(r_size) :: x_col(6, n)
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: words(:)
  INTEGER(c_int64_t), TARGET :: nrows, nbad, ninc, nw
  INTEGER(c_int64_t) :: nbytes
  TYPE(c_ptr) :: ctx, d_img, d_out
  TYPE(c_ptr), TARGET :: d_da(nmem)
  TYPE(c_ptr) :: d_elm, d_typ, d_lon, d_lat, d_lev, d_dat, d_err, d_dif, d_set, d_idx, d_qc, d_ens
  TYPE(letkf_obsfile_params) :: p
  TYPE(letkf_obsfile_cols) :: o
  TYPE(letkf_obsda_params) :: dp
  TYPE(letkf_obsda_cols) :: dc
  INTEGER :: i, k, m, u, ierr, nfail
  INTEGER(c_int) :: rc
  LOGICAL :: ok
  CHARACTER(len=512) :: dir

  CALL get_command_argument(1, dir)
  nfail = 0
  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')

  ! ---- the values: file units (hPa, percent), every id of the SELECT CASE that needs no projection, and an unknown one
  DO i = 1, n
    fil(1, i) = REAL(ids(MOD(i - 1, 9) + 1), r_sngl)
    fil(2, i) = 130.0 + 0.03125*i;  fil(3, i) = 30.0 + 0.0234375*i
    fil(4, i) = 1013.25 - 2.7*i;    fil(5, i) = 55.5 + 0.37*i;  fil(6, i) = 0.1 + 0.013*i
    fil(7, i) = REAL(MOD(i, 23) + 1, r_sngl);  fil(8, i) = -1800.0 + 12.0*i
    rad(1, i) = REAL(4001 + MOD(i, 2), r_sngl)
    rad(2:6, i) = fil(2:6, i) * 1.5;  rad(7, i) = 7.0
    DO m = 1, nmem
      da(1, i, m) = REAL(MOD(i, 3) + 1, r_sngl);  da(2, i, m) = REAL(i*7, r_sngl)
      da(3, i, m) = 0.001*i*m - 0.2;  da(4, i, m) = REAL(MERGE(10*m, 0, MOD(i + m, 11) == 0), r_sngl)
    END DO
  END DO
  fil(6, 6) = 1.0e-37                                                ! an RH row: 1e-37 * 0.01 is a denormal

  ! ---- 1a. conventional: WRITE(iunit) wk, the bytes to the device, decode
  OPEN (newunit=u, file=TRIM(dir)//'/conv.dat', form='unformatted', access='sequential', status='replace')
  DO i = 1, n
    wk = fil(:, i)
    WRITE (u) wk
  END DO
  CLOSE (u)
  CALL slurp(TRIM(dir)//'/conv.dat')
  CALL obsfile_count_amd(1, 8, nbytes, nrows, ierr)
  CALL report('conv_count', ierr == 0 .AND. nrows == n)
  DO i = 1, n                                                        ! read_obs (:2161-2206) on what was written
    wk = fil(:, i)
    SELECT CASE (NINT(wk(1)))
    CASE (2819, 2820, 3073, 3074, 3330)
      wk(4) = wk(4) * 100.0
    CASE (14593)
      wk(5) = wk(5) * 100.0
      wk(6) = wk(6) * 100.0
    CASE (3331)
      wk(4) = wk(4) * 100.0
      wk(5) = wk(5) * 0.01
      wk(6) = wk(6) * 0.01
    CASE (99993)
      wk(4) = wk(4) * 100.0
      wk(5) = wk(5) * 100.0
      wk(6) = REAL(5.0d2, kind=r_sngl)
    END SELECT
    x_elm(i) = NINT(wk(1));  x_typ(i) = NINT(wk(7))
    x_col(1, i) = REAL(wk(2), r_size);  x_col(2, i) = REAL(wk(3), r_size);  x_col(3, i) = REAL(wk(4), r_size)
    x_col(4, i) = REAL(wk(5), r_size);  x_col(5, i) = REAL(wk(6), r_size);  x_col(6, i) = REAL(wk(8), r_size)
  END DO
  CALL device_columns()
  p%format = LETKF_OBSFILE_CONV; p%nrec = 8; p%big_endian = 0; p%missing = 1; p%proj_given = 0; p%reserved0 = 0
  p%obserr_tcp = 5.0d2; p%obserr_tcx = 50.0d3; p%obserr_tcy = 50.0d3
  d_img = up(c_loc(words), nbytes)
  CALL obs_decode_amd(ctx, p, d_img, nrows, o, ierr, nbad=nbad)
  CALL chk(INT(ierr, c_int), 'obs_decode_amd conv')
  CALL fetch_columns()
  ok = nbad == 0 .AND. ALL(elm == x_elm) .AND. ALL(typ == x_typ) .AND. ALL(lon == x_col(1, :)) .AND. ALL(lat == x_col(2, :)) &
       .AND. ALL(lev == x_col(3, :)) .AND. ALL(dat == x_col(4, :)) .AND. ALL(err == x_col(5, :)) .AND. ALL(dif == x_col(6, :))
  CALL report('conv_decode', ok)
  CALL report('conv_denormal_kept', err(6) > 0.0d0 .AND. err(6) < REAL(TINY(1.0_r_sngl), r_size))

  ! ---- 2a. the columns back: encode on the device, the bytes to a file, sequential READ
  CALL chk(hipMalloc(d_out, INT(nbytes, c_size_t)), 'hipMalloc image')
  CALL obs_encode_amd(ctx, p, nrows, o, d_out, nw, ierr)
  CALL chk(INT(ierr, c_int), 'obs_encode_amd conv')
  CALL spit(TRIM(dir)//'/conv_dev.dat', d_out, nbytes)
  ok = nw == n
  OPEN (newunit=u, file=TRIM(dir)//'/conv_dev.dat', form='unformatted', access='sequential', status='old')
  DO i = 1, n
    READ (u, iostat=ierr) wk
    IF (ierr /= 0) ok = .FALSE.
    IF (ierr /= 0) EXIT
    CALL expected_write(i, wd)                                        ! wd(1:3) = lev, dat, err as write_obs writes them
    ok = ok .AND. wk(1) == REAL(x_elm(i), r_sngl) .AND. wk(2) == REAL(x_col(1, i), r_sngl) .AND. wk(3) == REAL(x_col(2, i), r_sngl) &
         .AND. wk(4) == wd(1) .AND. wk(5) == wd(2) .AND. wk(6) == wd(3) .AND. wk(7) == REAL(x_typ(i), r_sngl) &
         .AND. wk(8) == REAL(x_col(6, i), r_sngl)
  END DO
  READ (u, iostat=ierr) wk
  ok = ok .AND. ierr /= 0                                            ! and no record more
  CLOSE (u)
  CALL report('conv_encode', ok)

  ! ---- 1b. radar: three records of one value, then wk(1:7)
  OPEN (newunit=u, file=TRIM(dir)//'/radar.dat', form='unformatted', access='sequential', status='replace')
  WRITE (u) REAL(135.523d0, r_sngl)
  WRITE (u) REAL(34.823d0, r_sngl)
  WRITE (u) REAL(120.5d0, r_sngl)
  DO i = 1, n
    WRITE (u) rad(1:7, i)
  END DO
  CLOSE (u)
  CALL slurp(TRIM(dir)//'/radar.dat')
  CALL obsfile_count_amd(2, 7, nbytes, nrows, ierr)
  CALL report('radar_count', ierr == 0 .AND. nrows == n)
  p%format = LETKF_OBSFILE_RADAR; p%nrec = 7
  d_img = up(c_loc(words), nbytes)
  CALL obs_decode_amd(ctx, p, d_img, nrows, o, ierr, meta=meta, nbad=nbad)
  CALL chk(INT(ierr, c_int), 'obs_decode_amd radar')
  CALL fetch_columns()
  ok = nbad == 0 .AND. ALL(elm == NINT(rad(1, :))) .AND. ALL(typ == 22) .AND. ALL(dif == 0.0d0)
  ok = ok .AND. ALL(lon == REAL(rad(2, :), r_size)) .AND. ALL(lat == REAL(rad(3, :), r_size)) .AND. ALL(lev == REAL(rad(4, :), r_size))
  ok = ok .AND. ALL(dat == REAL(rad(5, :), r_size)) .AND. ALL(err == REAL(rad(6, :), r_size))
  ok = ok .AND. meta(1) == REAL(REAL(135.523d0, r_sngl), r_size) .AND. meta(2) == REAL(REAL(34.823d0, r_sngl), r_size) .AND. meta(3) == 120.5d0
  CALL report('radar_decode', ok)

  ! ---- 2b. radar back, without the undefined rows: every seventh dat is undef
  DO i = 7, n, 7
    dat(i) = -9.99d33
  END DO
  CALL chk(hipMemcpy(d_dat, c_loc(dat), 8_c_size_t*n, hipMemcpyHostToDevice), 'upload dat')
  p%missing = 0
  CALL chk(hipMalloc(d_out, INT(nbytes, c_size_t)), 'hipMalloc image')
  CALL obs_encode_amd(ctx, p, nrows, o, d_out, nw, ierr, meta=meta)
  CALL chk(INT(ierr, c_int), 'obs_encode_amd radar')
  ok = nw == n - n/7
  CALL spit(TRIM(dir)//'/radar_dev.dat', d_out, 36_c_int64_t + 36_c_int64_t*nw)
  OPEN (newunit=u, file=TRIM(dir)//'/radar_dev.dat', form='unformatted', access='sequential', status='old')
  READ (u) tmp;  ok = ok .AND. tmp == REAL(135.523d0, r_sngl)
  READ (u) tmp;  ok = ok .AND. tmp == REAL(34.823d0, r_sngl)
  READ (u) tmp;  ok = ok .AND. tmp == 120.5
  DO i = 1, n
    IF (MOD(i, 7) == 0) CYCLE
    READ (u, iostat=ierr) wk(1:7)
    IF (ierr /= 0) ok = .FALSE.
    IF (ierr /= 0) EXIT
    ok = ok .AND. ALL(wk(1:6) == rad(1:6, i)) .AND. wk(7) == 22.0
  END DO
  READ (u, iostat=ierr) wk(1:7)
  ok = ok .AND. ierr /= 0
  CLOSE (u)
  CALL report('radar_encode_without_undefined', ok)

  ! ---- 1c. obsda: one file per member, assembled into ensval(member, row)
  DO m = 1, nmem
    OPEN (newunit=u, file=TRIM(dir)//'/obsda'//ACHAR(48 + m)//'.dat', form='unformatted', access='sequential', status='replace')
    DO i = 1, n
      wd = da(:, i, m)
      WRITE (u) wd
    END DO
    CLOSE (u)
    CALL slurp(TRIM(dir)//'/obsda'//ACHAR(48 + m)//'.dat')
    d_da(m) = up(c_loc(words), nbytes)
    col(m) = nmem - m                                                ! member m into column nmem - m (0-based)
  END DO
  CALL obsfile_count_amd(3, 4, nbytes, nrows, ierr)
  CALL report('obsda_count', ierr == 0 .AND. nrows == n)
  set = 0; idx = 0; qc = 0; ensval = -1.0d0
  d_set = up(c_loc(set), 4_c_int64_t*n); d_idx = up(c_loc(idx), 4_c_int64_t*n); d_qc = up(c_loc(qc), 4_c_int64_t*n)
  d_ens = up(c_loc(ensval), 8_c_int64_t*n*nmem)
  dp%nrec = 4; dp%big_endian = 0; dp%nmem = nmem; dp%finish = 0; dp%member = nmem; dp%reserved0 = 0; dp%nobs = n; dp%kld = nmem
  dc%set = d_set; dc%idx = d_idx; dc%qc = d_qc; dc%ensval = d_ens; dc%lev = c_null_ptr; dc%val2 = c_null_ptr
  CALL obsda_assemble_amd(ctx, dp, d_da, col, dc, ierr, ninconsistent=ninc, nbad=nbad)
  CALL chk(INT(ierr, c_int), 'obsda_assemble_amd')
  CALL chk(hipMemcpy(c_loc(set), d_set, 4_c_size_t*n, hipMemcpyDeviceToHost), 'download set')
  CALL chk(hipMemcpy(c_loc(idx), d_idx, 4_c_size_t*n, hipMemcpyDeviceToHost), 'download idx')
  CALL chk(hipMemcpy(c_loc(qc), d_qc, 4_c_size_t*n, hipMemcpyDeviceToHost), 'download qc')
  CALL chk(hipMemcpy(c_loc(ensval), d_ens, 8_c_size_t*n*nmem, hipMemcpyDeviceToHost), 'download ensval')
  ok = ninc == 0 .AND. nbad == 0
  DO i = 1, n
    x_qc(i) = MAX(0, NINT(da(4, i, 1)), NINT(da(4, i, 2)), NINT(da(4, i, 3)))
    ok = ok .AND. set(i) == NINT(da(1, i, 1)) .AND. idx(i) == NINT(da(2, i, 1)) .AND. qc(i) == x_qc(i)
    DO m = 1, nmem
      ok = ok .AND. ensval(nmem - m + 1, i) == REAL(da(3, i, m), r_size)
    END DO
  END DO
  CALL report('obsda_assemble', ok)

  ! ---- 2c. write_obs_da of member 2's column on the device, read back with READ(iunit) wk
  CALL chk(hipMalloc(d_out, INT(nbytes, c_size_t)), 'hipMalloc image')
  CALL obsda_encode_amd(ctx, 4, nrows, d_set, d_idx, d_qc, d_ens, INT(nmem, c_int64_t), nmem - 2, c_null_ptr, c_null_ptr, c_null_ptr, &
                        d_out, ierr)
  CALL chk(INT(ierr, c_int), 'obsda_encode_amd')
  CALL spit(TRIM(dir)//'/obsda_dev.dat', d_out, nbytes)
  ok = .TRUE.
  OPEN (newunit=u, file=TRIM(dir)//'/obsda_dev.dat', form='unformatted', access='sequential', status='old')
  DO i = 1, n
    READ (u, iostat=ierr) wd
    IF (ierr /= 0) ok = .FALSE.
    IF (ierr /= 0) EXIT
    ok = ok .AND. wd(1) == da(1, i, 2) .AND. wd(2) == da(2, i, 2) .AND. wd(3) == da(3, i, 2) .AND. wd(4) == REAL(x_qc(i), r_sngl)
  END DO
  READ (u, iostat=ierr) wd
  ok = ok .AND. ierr /= 0
  CLOSE (u)
  CALL report('obsda_encode', ok)

  rc = letkf_ctx_destroy(ctx)
  IF (nfail > 0) STOP 1

CONTAINS

  ! write_obs' SELECT CASE (:2245-2266) on row i of the decoded columns: w(1:3) = wk(4:6)
  SUBROUTINE expected_write(i_, w)
    INTEGER, INTENT(IN) :: i_
    REAL(r_sngl), INTENT(OUT) :: w(4)
    w(1) = REAL(x_col(3, i_), r_sngl);  w(2) = REAL(x_col(4, i_), r_sngl);  w(3) = REAL(x_col(5, i_), r_sngl);  w(4) = 0.0
    SELECT CASE (x_elm(i_))
    CASE (2819, 2820, 3073, 3074, 3330)
      w(1) = w(1) * 0.01
    CASE (14593, 99993)
      w(2) = w(2) * 0.01
      w(3) = w(3) * 0.01
    CASE (3331)
      w(1) = w(1) * 0.01
      w(2) = w(2) * 100.0
      w(3) = w(3) * 100.0
    END SELECT
  END SUBROUTINE expected_write

  ! a file's bytes, as they are, into words / nbytes
  SUBROUTINE slurp(name)
    CHARACTER(*), INTENT(IN) :: name
    INTEGER :: v
    INQUIRE (file=name, size=nbytes)
    IF (ALLOCATED(words)) DEALLOCATE (words)
    ALLOCATE (words(MAX(nbytes/4, 1_c_int64_t)))
    OPEN (newunit=v, file=name, access='stream', form='unformatted', status='old')
    IF (nbytes > 0) READ (v) words(1:nbytes/4)
    CLOSE (v)
  END SUBROUTINE slurp

  ! nb bytes of a device image into a file, as they are
  SUBROUTINE spit(name, d, nb)
    CHARACTER(*), INTENT(IN) :: name
    TYPE(c_ptr), INTENT(IN) :: d
    INTEGER(c_int64_t), INTENT(IN) :: nb
    INTEGER :: v
    CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
    IF (ALLOCATED(words)) DEALLOCATE (words)
    ALLOCATE (words(MAX(nb/4, 1_c_int64_t)))
    CALL chk(hipMemcpy(c_loc(words), d, INT(nb, c_size_t), hipMemcpyDeviceToHost), 'download image')
    OPEN (newunit=v, file=name, access='stream', form='unformatted', status='replace')
    WRITE (v) words(1:nb/4)
    CLOSE (v)
  END SUBROUTINE spit

  SUBROUTINE device_columns()
    elm = -1; typ = -1; lon = -1.0d0; lat = -1.0d0; lev = -1.0d0; dat = -1.0d0; err = -1.0d0; dif = -1.0d0
    d_elm = up(c_loc(elm), 4_c_int64_t*n); d_typ = up(c_loc(typ), 4_c_int64_t*n)
    d_lon = up(c_loc(lon), 8_c_int64_t*n); d_lat = up(c_loc(lat), 8_c_int64_t*n); d_lev = up(c_loc(lev), 8_c_int64_t*n)
    d_dat = up(c_loc(dat), 8_c_int64_t*n); d_err = up(c_loc(err), 8_c_int64_t*n); d_dif = up(c_loc(dif), 8_c_int64_t*n)
    o%elm = d_elm; o%typ = d_typ; o%lon = d_lon; o%lat = d_lat; o%lev = d_lev; o%dat = d_dat; o%err = d_err; o%dif = d_dif
  END SUBROUTINE device_columns

  SUBROUTINE fetch_columns()
    CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
    CALL chk(hipMemcpy(c_loc(elm), d_elm, 4_c_size_t*n, hipMemcpyDeviceToHost), 'download elm')
    CALL chk(hipMemcpy(c_loc(typ), d_typ, 4_c_size_t*n, hipMemcpyDeviceToHost), 'download typ')
    CALL chk(hipMemcpy(c_loc(lon), d_lon, 8_c_size_t*n, hipMemcpyDeviceToHost), 'download lon')
    CALL chk(hipMemcpy(c_loc(lat), d_lat, 8_c_size_t*n, hipMemcpyDeviceToHost), 'download lat')
    CALL chk(hipMemcpy(c_loc(lev), d_lev, 8_c_size_t*n, hipMemcpyDeviceToHost), 'download lev')
    CALL chk(hipMemcpy(c_loc(dat), d_dat, 8_c_size_t*n, hipMemcpyDeviceToHost), 'download dat')
    CALL chk(hipMemcpy(c_loc(err), d_err, 8_c_size_t*n, hipMemcpyDeviceToHost), 'download err')
    CALL chk(hipMemcpy(c_loc(dif), d_dif, 8_c_size_t*n, hipMemcpyDeviceToHost), 'download dif')
  END SUBROUTINE fetch_columns

  FUNCTION up(host, nb) RESULT(d)
    TYPE(c_ptr), INTENT(IN) :: host
    INTEGER(c_int64_t), INTENT(IN) :: nb
    TYPE(c_ptr) :: d
    CALL chk(hipMalloc(d, INT(MAX(nb, 8_c_int64_t), c_size_t)), 'hipMalloc')
    IF (nb > 0) CALL chk(hipMemcpy(d, host, INT(nb, c_size_t), hipMemcpyHostToDevice), 'hipMemcpy H2D')
  END FUNCTION up

  SUBROUTINE report(what, passed)
    CHARACTER(*), INTENT(IN) :: what
    LOGICAL, INTENT(IN) :: passed
    IF (passed) THEN
      WRITE (6, '(2A)') 'PASS ', what
    ELSE
      WRITE (6, '(2A)') 'FAIL ', what
      nfail = nfail + 1
    END IF
  END SUBROUTINE report

  SUBROUTINE chk(rc_, what)
    INTEGER(c_int), INTENT(IN) :: rc_
    CHARACTER(*), INTENT(IN) :: what
    IF (rc_ /= 0) THEN
      WRITE (6, *) 'FAIL error', rc_, 'in ', what
      STOP 5
    END IF
  END SUBROUTINE chk

END PROGRAM obsfile_driver
