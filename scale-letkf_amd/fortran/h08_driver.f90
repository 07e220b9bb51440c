!===============================================================================
! h08_driver.f90 -- the Himawari-8 radiances called from Fortran (INTEGRATION.md), in two parts.
!   1. The record framing against Fortran's own I/O, as obsfile_driver checks the other formats: WRITE(iunit) wk(4+nch) into a file
!      (FORM='unformatted', ACCESS='sequential'), its bytes read with ACCESS='stream', letkf_h08_count and letkf_h08_decode_dev,
!      the columns compared with read_obs_H08's; then letkf_h08_encode_dev, the bytes written with ACCESS='stream' and read back
!      with sequential READ(iunit) wk.  One PASS / FAIL line per check.
!   2. A case written by tests/test_fortran_h08.py through letkf_h08_select_dev, letkf_h08_profiles_dev, a STAND-IN for the host's
!      radiative transfer (not a product: tau = exp(-(p / pc)**2) per channel, brightness temperatures from it and from the cloud
!      column) and letkf_h08_rows_dev; everything the entries and the stand-in gave is written for the test to compare.
!   case file (little endian, stream):
!     int32 nlev, khalo, nlon, nlat, ihalo, jhalo, nmem, nprof, nrow, kld, m0, h08_set ; letkf_h08_params (its C bytes)
!     real64 v3d(nlevh, nlonh, nlath, 13, nmem), v2d(nlonh, nlath, 9, nmem)
!     real64 ri(nprof), rj(nprof), lon(nprof), lat(nprof), rotc(2, nprof)
!     int32 set(nrow), idx(nrow), qc(nrow) ; real64 ensval(kld, nrow), lev(nrow), val2(nrow)
!   output: int64 nsel ; int32 prof_list(nprof), slot_of_prof(nprof) ; real64 lev3(nlev, 5, nsel, nmem), sfc(8, nsel, nmem) ;
!     int32 pflag(nsel) ; real64 btall(10, nsel, nmem), btclr(10, nsel, nmem), trans(nlev, 10, nsel, nmem) ;
!     int32 qc(nrow) ; real64 ensval(kld, nrow), lev(nrow), val2(nrow)
! Arguments: a directory to write into, the case file, the output file.
!===============================================================================
PROGRAM h08_driver
  USE letkf_h08_amd
  IMPLICIT NONE
  INTEGER, PARAMETER :: np = 130, nch = 10, r_sngl = c_float, r_size = c_double
  REAL(r_sngl) :: wk(4 + nch), rec(4 + nch, np)
  REAL(r_size), TARGET :: obserr(nch)
  INTEGER(c_int32_t), TARGET :: elm(np*nch), typ(np*nch)
  REAL(r_size), TARGET :: col(np*nch, 6)                             ! lon, lat, lev, dat, err, dif
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: words(:)
  INTEGER(c_int64_t), TARGET :: nbad
  INTEGER(c_int64_t) :: nprof_file, nbytes
  TYPE(c_ptr) :: ctx, d_img, d_out, d_elm, d_typ, d_col(6)
  TYPE(letkf_obsfile_cols) :: o
  INTEGER :: i, c, k, u, n, nfail
  INTEGER(c_int) :: rc
  LOGICAL :: ok
  CHARACTER(len=512) :: dir, fin, fout

  CALL get_command_argument(1, dir)
  CALL get_command_argument(2, fin)
  CALL get_command_argument(3, fout)
  nfail = 0
  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')

  ! ---- 1a. WRITE(iunit) wk, the bytes to the device, count and decode
  DO i = 1, np
    rec(1, i) = 8800.0;  rec(2, i) = 23.0
    rec(3, i) = 120.0 + 0.3125*i;  rec(4, i) = -40.0 + 0.61*i
    DO c = 1, nch
      rec(4 + c, i) = 200.0 + 0.37*i + 3.1*c
    END DO
  END DO
  rec(1, 7) = 8799.5;  rec(2, 7) = -22.5                             ! NINT: half away from zero
  DO c = 1, nch
    obserr(c) = 1.5d0 + 0.25d0*c
  END DO
  OPEN (newunit=u, file=TRIM(dir)//'/h08.dat', form='unformatted', access='sequential', status='replace')
  DO i = 1, np
    wk = rec(:, i)
    WRITE (u) wk
  END DO
  CLOSE (u)
  CALL slurp(TRIM(dir)//'/h08.dat')
  nbytes = 4_c_int64_t*SIZE(words)
  CALL chk(letkf_h08_count(nbytes, nprof_file), 'h08_count')
  CALL report('h08_count', nprof_file == np .AND. nbytes == 64*np)
  d_img = up(c_loc(words), INT(nbytes, c_size_t))
  n = np*nch
  CALL chk(hipMalloc(d_elm, 4_c_size_t*n), 'hipMalloc');  CALL chk(hipMalloc(d_typ, 4_c_size_t*n), 'hipMalloc')
  DO k = 1, 6
    CALL chk(hipMalloc(d_col(k), 8_c_size_t*n), 'hipMalloc')
  END DO
  o%elm = d_elm; o%typ = d_typ; o%lon = d_col(1); o%lat = d_col(2); o%lev = d_col(3); o%dat = d_col(4); o%err = d_col(5); o%dif = d_col(6)
  CALL chk(letkf_h08_decode_dev(ctx, 0_c_int32_t, d_img, nprof_file, obserr, o, c_loc(nbad)), 'h08_decode')
  CALL chk(hipMemcpy(c_loc(elm), d_elm, 4_c_size_t*n, hipMemcpyDeviceToHost), 'download')
  CALL chk(hipMemcpy(c_loc(typ), d_typ, 4_c_size_t*n, hipMemcpyDeviceToHost), 'download')
  DO k = 1, 6
    CALL chk(hipMemcpy(c_loc(col(1, k)), d_col(k), 8_c_size_t*n, hipMemcpyDeviceToHost), 'download')
  END DO
  ok = nbad == 0
  DO i = 1, np                                                       ! read_obs_H08 (common_obs_scale.f90:3052-3069)
    DO c = 1, nch
      k = (i - 1)*nch + c
      ok = ok .AND. elm(k) == NINT(rec(1, i)) .AND. typ(k) == NINT(rec(2, i))
      ok = ok .AND. col(k, 1) == REAL(rec(3, i), r_size) .AND. col(k, 2) == REAL(rec(4, i), r_size)
      ok = ok .AND. col(k, 3) == c + 6.0 .AND. col(k, 4) == REAL(rec(4 + c, i), r_size)
      ok = ok .AND. col(k, 5) == obserr(c) .AND. col(k, 6) == 0.0d0
    END DO
  END DO
  CALL report('h08_decode', ok .AND. elm((7 - 1)*nch + 1) == 8800 .AND. typ((7 - 1)*nch + 1) == -23)

  ! ---- 1b. encode on the device, the bytes to a file, READ(iunit) wk
  CALL chk(hipMalloc(d_out, INT(nbytes, c_size_t)), 'hipMalloc')
  CALL chk(letkf_h08_encode_dev(ctx, 0_c_int32_t, nprof_file, o, d_out), 'h08_encode')
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
  CALL spit(TRIM(dir)//'/h08_dev.dat', d_out, INT(nbytes, c_size_t))
  OPEN (newunit=u, file=TRIM(dir)//'/h08_dev.dat', form='unformatted', access='sequential', status='old')
  ok = .TRUE.
  DO i = 1, np                                                       ! write_obs_H08 (:3098-3104) of the decoded columns
    READ (u) wk
    ok = ok .AND. wk(1) == REAL(NINT(rec(1, i)), r_sngl) .AND. wk(2) == REAL(NINT(rec(2, i)), r_sngl)
    ok = ok .AND. ALL(wk(3:) == rec(3:, i))
  END DO
  CLOSE (u)
  CALL report('h08_encode', ok)

  ! ---- 2. the case of the test
  CALL run_case()
  rc = letkf_ctx_destroy(ctx)
  IF (nfail > 0) STOP 4

CONTAINS

  SUBROUTINE run_case()
    INTEGER(c_int32_t) :: nlev, khalo, nlon, nlat, ihalo, jhalo, nmem, nprof, nrow, kld, m0, h08_set
    INTEGER(c_int64_t) :: nlevh, nlonh, nlath, nsel
    TYPE(letkf_h08_params) :: p
    TYPE(letkf_obsope_fields) :: f
    TYPE(letkf_h08_profiles) :: out
    REAL(r_size), ALLOCATABLE, TARGET :: v3d(:, :, :, :, :), v2d(:, :, :, :), ri(:), rj(:), lon(:), lat(:), rotc(:, :)
    REAL(r_size), ALLOCATABLE, TARGET :: ensval(:, :), lev(:), val2(:), lev3(:, :, :, :), sfc(:, :, :)
    REAL(r_size), ALLOCATABLE, TARGET :: btall(:, :, :), btclr(:, :, :), trans(:, :, :, :)
    INTEGER(c_int32_t), ALLOCATABLE, TARGET :: set(:), idx(:), qc(:), prof_list(:), slot(:), pflag(:)
    TYPE(c_ptr) :: d_v3, d_v2, d_ri, d_rj, d_lon, d_lat, d_rotc, d_set, d_idx, d_qc, d_ens, d_lev, d_val2, d_pl, d_slot
    TYPE(c_ptr) :: d_lev3, d_sfc, d_cloud, d_pflag, d_btall, d_btclr, d_trans
    INTEGER :: ios, v

    OPEN (newunit=v, file=TRIM(fin), access='stream', form='unformatted', status='old', iostat=ios)
    IF (ios /= 0) STOP 3
    READ (v) nlev, khalo, nlon, nlat, ihalo, jhalo, nmem, nprof, nrow, kld, m0, h08_set
    READ (v) p
    nlevh = nlev + 2*khalo;  nlonh = nlon + 2*ihalo;  nlath = nlat + 2*jhalo
    ALLOCATE (v3d(nlevh, nlonh, nlath, 13, nmem), v2d(nlonh, nlath, 9, nmem), ri(nprof), rj(nprof), lon(nprof), lat(nprof))
    ALLOCATE (rotc(2, nprof), set(nrow), idx(nrow), qc(nrow), ensval(kld, nrow), lev(nrow), val2(nrow), prof_list(nprof), slot(nprof))
    READ (v) v3d, v2d
    READ (v) ri, rj, lon, lat, rotc
    READ (v) set, idx, qc
    READ (v) ensval, lev, val2
    CLOSE (v)
    d_v3 = up(c_loc(v3d), 8_c_size_t*SIZE(v3d));  d_v2 = up(c_loc(v2d), 8_c_size_t*SIZE(v2d))
    d_ri = up(c_loc(ri), 8_c_size_t*nprof);  d_rj = up(c_loc(rj), 8_c_size_t*nprof)
    d_lon = up(c_loc(lon), 8_c_size_t*nprof);  d_lat = up(c_loc(lat), 8_c_size_t*nprof)
    d_rotc = up(c_loc(rotc), 16_c_size_t*nprof)
    d_set = up(c_loc(set), 4_c_size_t*nrow);  d_idx = up(c_loc(idx), 4_c_size_t*nrow);  d_qc = up(c_loc(qc), 4_c_size_t*nrow)
    d_ens = up(c_loc(ensval), 8_c_size_t*kld*nrow)
    d_lev = up(c_loc(lev), 8_c_size_t*nrow);  d_val2 = up(c_loc(val2), 8_c_size_t*nrow)
    prof_list = -1
    d_pl = up(c_loc(prof_list), 4_c_size_t*nprof);  d_slot = up(c_loc(slot), 4_c_size_t*nprof)

    ! which profiles of the file the rows name
    CALL chk(letkf_h08_select_dev(ctx, d_set, d_idx, 0_c_int64_t, INT(nrow, c_int64_t), h08_set, INT(nprof, c_int64_t), d_pl, &
                                  d_slot, nsel), 'h08_select')
    ALLOCATE (lev3(nlev, 5, nsel, nmem), sfc(8, nsel, nmem), pflag(nsel), btall(nch, nsel, nmem), btclr(nch, nsel, nmem))
    ALLOCATE (trans(nlev, nch, nsel, nmem))

    ! the profile arrays of every member, in the reference's layout per member
    f%nlev = nlev; f%nlon = nlon; f%nlat = nlat; f%khalo = khalo; f%ihalo = ihalo; f%jhalo = jhalo
    f%nv3dd = 13; f%nv2dd = 9; f%nmem = nmem; f%m0 = 0
    f%v3d = d_v3; f%s3k = 1; f%s3i = nlevh; f%s3j = nlevh*nlonh; f%s3v = nlevh*nlonh*nlath; f%s3m = 13*nlevh*nlonh*nlath
    f%v2d = d_v2; f%s2i = 1; f%s2j = nlonh; f%s2v = nlonh*nlath; f%s2m = 9*nlonh*nlath
    CALL chk(hipMalloc(d_lev3, 8_c_size_t*SIZE(lev3)), 'hipMalloc');  CALL chk(hipMalloc(d_sfc, 8_c_size_t*SIZE(sfc)), 'hipMalloc')
    CALL chk(hipMalloc(d_cloud, 8_c_size_t*3*MAX(nlev - 1, 1)*nsel*nmem), 'hipMalloc')
    CALL chk(hipMalloc(d_pflag, 4_c_size_t*MAX(nsel, 1_c_int64_t)), 'hipMalloc')
    out%lev3 = d_lev3; out%sfc = d_sfc; out%cloud = d_cloud; out%pflag = d_pflag
    CALL chk(letkf_h08_profiles_dev(ctx, p, f, nsel, d_pl, d_ri, d_rj, d_lon, d_lat, d_rotc, out), 'h08_profiles')
    CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
    CALL chk(hipMemcpy(c_loc(lev3), d_lev3, 8_c_size_t*SIZE(lev3), hipMemcpyDeviceToHost), 'download lev3')
    CALL chk(hipMemcpy(c_loc(sfc), d_sfc, 8_c_size_t*SIZE(sfc), hipMemcpyDeviceToHost), 'download sfc')

    ! where the host calls RTTOV
    CALL stand_in(p, nlev, INT(nsel), nmem, lev3, sfc, btall, btclr, trans)
    d_btall = up(c_loc(btall), 8_c_size_t*SIZE(btall));  d_btclr = up(c_loc(btclr), 8_c_size_t*SIZE(btclr))
    d_trans = up(c_loc(trans), 8_c_size_t*SIZE(trans))

    ! the obsda rows; rig / rjg are ri / rj: one subdomain
    CALL chk(letkf_h08_rows_dev(ctx, p, 0_c_int64_t, INT(nrow, c_int64_t), d_set, d_idx, h08_set, d_slot, nsel, nmem, m0, d_lev3, &
                                d_sfc, d_pflag, d_btall, d_btclr, d_trans, d_ri, d_rj, 1_c_int32_t, d_qc, d_ens, &
                                INT(kld, c_int64_t), d_lev, d_val2), 'h08_rows')
    CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
    CALL chk(hipMemcpy(c_loc(prof_list), d_pl, 4_c_size_t*nprof, hipMemcpyDeviceToHost), 'download')
    CALL chk(hipMemcpy(c_loc(slot), d_slot, 4_c_size_t*nprof, hipMemcpyDeviceToHost), 'download')
    CALL chk(hipMemcpy(c_loc(pflag), d_pflag, 4_c_size_t*nsel, hipMemcpyDeviceToHost), 'download')
    CALL chk(hipMemcpy(c_loc(qc), d_qc, 4_c_size_t*nrow, hipMemcpyDeviceToHost), 'download')
    CALL chk(hipMemcpy(c_loc(ensval), d_ens, 8_c_size_t*kld*nrow, hipMemcpyDeviceToHost), 'download')
    CALL chk(hipMemcpy(c_loc(lev), d_lev, 8_c_size_t*nrow, hipMemcpyDeviceToHost), 'download')
    CALL chk(hipMemcpy(c_loc(val2), d_val2, 8_c_size_t*nrow, hipMemcpyDeviceToHost), 'download')
    OPEN (newunit=v, file=TRIM(fout), access='stream', form='unformatted', status='replace')
    WRITE (v) nsel, prof_list, slot, lev3, sfc, pflag, btall, btclr, trans, qc, ensval, lev, val2
    CLOSE (v)
    CALL report('h08_case', nsel > 0)
  END SUBROUTINE run_case

  ! NOT a radiative transfer: a smooth function of the profile arrays, in their level order
  SUBROUTINE stand_in(p, nlev, nsel, nmem, lev3, sfc, btall, btclr, trans)
    TYPE(letkf_h08_params), INTENT(IN) :: p
    INTEGER, INTENT(IN) :: nlev, nsel, nmem
    REAL(r_size), INTENT(IN) :: lev3(nlev, 5, nsel, nmem), sfc(8, nsel, nmem)
    REAL(r_size), INTENT(OUT) :: btall(nch, nsel, nmem), btclr(nch, nsel, nmem), trans(nlev, nch, nsel, nmem)
    REAL(r_size) :: tau(nlev), prs(nlev), t(nlev), pc, cld, bt
    INTEGER :: m, s, cc, kk, l
    DO m = 1, nmem
      DO s = 1, nsel
        DO kk = 1, nlev                                              ! kk: model order, bottom up
          l = MERGE(nlev + 1 - kk, kk, p%top_down /= 0)
          prs(kk) = lev3(l, 1, s, m)*MERGE(100.0d0, 1.0d0, p%rttov_units /= 0)
          t(kk) = lev3(l, 2, s, m)
        END DO
        cld = SUM(lev3(:, 4, s, m) + lev3(:, 5, s, m))
        DO cc = 1, nch
          pc = 50.0d3 + 4.0d3*(cc - 1)
          tau = EXP(-(prs/pc)**2)
          bt = tau(1)*sfc(1, s, m) + (1.0d0 - tau(nlev))*210.0d0
          DO kk = 2, nlev
            bt = bt + (tau(kk) - tau(kk - 1))*0.5d0*(t(kk) + t(kk - 1))
          END DO
          btclr(cc, s, m) = bt
          btall(cc, s, m) = bt - (2.0d0 + 0.3d0*(cc - 1))*(1.0d0 - EXP(-cld/4.0d-3))
          DO kk = 1, nlev
            l = MERGE(nlev + 1 - kk, kk, p%top_down /= 0)
            trans(l, cc, s, m) = tau(kk)
          END DO
        END DO
      END DO
    END DO
  END SUBROUTINE stand_in

  ! a file's bytes into words(:)
  SUBROUTINE slurp(name)
    CHARACTER(*), INTENT(IN) :: name
    INTEGER :: v, sz
    INQUIRE (file=name, size=sz)
    IF (ALLOCATED(words)) DEALLOCATE (words)
    ALLOCATE (words(sz/4))
    OPEN (newunit=v, file=name, access='stream', form='unformatted', status='old')
    READ (v) words
    CLOSE (v)
  END SUBROUTINE slurp

  ! nb bytes of device memory into a file
  SUBROUTINE spit(name, d, nb)
    CHARACTER(*), INTENT(IN) :: name
    TYPE(c_ptr), INTENT(IN) :: d
    INTEGER(c_size_t), INTENT(IN) :: nb
    INTEGER(c_int32_t), ALLOCATABLE, TARGET :: w(:)
    INTEGER :: v
    ALLOCATE (w(nb/4))
    CALL chk(hipMemcpy(c_loc(w), d, nb, hipMemcpyDeviceToHost), 'hipMemcpy D2H')
    OPEN (newunit=v, file=name, access='stream', form='unformatted', status='replace')
    WRITE (v) w
    CLOSE (v)
  END SUBROUTINE spit

  FUNCTION up(host, nb) RESULT(d)
    TYPE(c_ptr), INTENT(IN) :: host
    INTEGER(c_size_t), INTENT(IN) :: nb
    TYPE(c_ptr) :: d
    CALL chk(hipMalloc(d, MAX(nb, 8_c_size_t)), 'hipMalloc')
    IF (nb > 0) CALL chk(hipMemcpy(d, host, nb, hipMemcpyHostToDevice), 'hipMemcpy H2D')
  END FUNCTION up

  SUBROUTINE report(what, passed)
    CHARACTER(*), INTENT(IN) :: what
    LOGICAL, INTENT(IN) :: passed
    IF (passed) THEN
      WRITE (6, '(A,1X,A)') 'PASS', what
    ELSE
      WRITE (6, '(A,1X,A)') 'FAIL', what
      nfail = nfail + 1
    END IF
  END SUBROUTINE report

  SUBROUTINE chk(rc_, what)
    INTEGER(c_int), INTENT(IN) :: rc_
    CHARACTER(*), INTENT(IN) :: what
    IF (rc_ /= 0) THEN
      WRITE (6, *) 'error', rc_, 'in ', what
      STOP 5
    END IF
  END SUBROUTINE chk

END PROGRAM h08_driver
