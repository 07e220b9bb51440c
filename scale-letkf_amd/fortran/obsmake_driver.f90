!===============================================================================
! obsmake_driver.f90 -- obsmake_cal from a Fortran host with the nature run on the device: dat zeroed, CALL obsmake_slot_amd
! per time slot on that slot's history fields, then CALL rand_create_amd and CALL obsmake_noise_amd (one subdomain: the
! MPI_REDUCE between them is the identity).  Reads a case written by tests/test_fortran_obsmake.py, writes the counts of every
! slot, dat before the noise, and dat and err after it.
!   file layout (little endian, stream):
!     int32 nlev, nlon, nlat, khalo, ihalo, jhalo, nfile, nrowf, nobtype, method, use_tv, stggrd, nradar, nslot, outside_undef,
!           seed (< 0: the clock's, as com_randn), has_own, 0, 0, 0
!     real64 min_radar_ref_dbz, low_ref_shift, radar_zmax, ps_adjust_thres, ri_off, rj_off, slot_lb of slot 1, SLOT_TINTERVAL
!     real64 obserr_u, v, t, q, rh, ps, radar_ref, radar_vr
!     int64 off(nfile+1) ; int32 file_radar(nfile) ; real64 radar_meta(3,nradar) ; int32 use_obs(nobtype)
!     int32 elm(nrowf), typ(nrowf) ; real64 lev, ri, rj, lon, lat, err, dif (nrowf each), rotc(2,nrowf) ; int32 own(nrowf)
!     per slot: real64 v3d(nlevh,nlonh,nlath,13), v2d(nlonh,nlath,7)
!   output: int64 counts(2,nslot) ; real64 dat(nrowf) before the noise ; real64 dat(nrowf), err(nrowf) after it
!===============================================================================
PROGRAM obsmake_driver
  USE letkf_obsmake_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: h(20)
  REAL(c_double) :: r(8), oe(8)
  INTEGER(c_int64_t), ALLOCATABLE, TARGET :: off(:), counts(:, :)
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: file_radar(:), use_obs(:), elm(:), typ(:), own(:)
  REAL(c_double), ALLOCATABLE, TARGET :: radar_meta(:, :), lev(:), ri(:), rj(:), lon(:), lat(:), dat(:), err(:), dif(:), rotc(:, :), &
                                         v3(:, :, :, :), v2(:, :, :)
  INTEGER :: u, uo, ios, nlev, nlon, nlat, khalo, ihalo, jhalo, nfile, nrowf, nobtype, nradar, nslot, nlevh, nlonh, nlath, ierr, &
             islot, seed, idate(8)
  INTEGER(c_int) :: rc
  TYPE(c_ptr) :: ctx, rand, d_elm, d_typ, d_lev, d_ri, d_rj, d_lon, d_lat, d_dat, d_err, d_dif, d_rotc, d_own, d_v3, d_v2, d_counts
  TYPE(letkf_obsope_params) :: prm
  TYPE(letkf_obsope_fields) :: fl
  TYPE(letkf_obsmake_slot) :: slot
  TYPE(letkf_obsmake_err) :: errs
  CHARACTER(len=512) :: fin, fout

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) h
  READ (u) r
  READ (u) oe
  nlev = h(1); nlon = h(2); nlat = h(3); khalo = h(4); ihalo = h(5); jhalo = h(6); nfile = h(7); nrowf = h(8)
  nobtype = h(9); nradar = h(13); nslot = h(14); seed = h(16)
  nlevh = nlev + 2*khalo; nlonh = nlon + 2*ihalo; nlath = nlat + 2*jhalo
  ALLOCATE (off(nfile + 1), file_radar(nfile), radar_meta(3, MAX(nradar, 1)), use_obs(nobtype), elm(nrowf), typ(nrowf), &
            lev(nrowf), ri(nrowf), rj(nrowf), lon(nrowf), lat(nrowf), dat(nrowf), err(nrowf), dif(nrowf), rotc(2, nrowf), &
            own(nrowf), v3(nlevh, nlonh, nlath, 13), v2(nlonh, nlath, 7), counts(2, nslot))
  READ (u) off, file_radar
  IF (nradar > 0) READ (u) radar_meta
  READ (u) use_obs, elm, typ, lev, ri, rj, lon, lat, err, dif, rotc, own

  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  d_elm = up(c_loc(elm), 4_c_size_t*nrowf); d_typ = up(c_loc(typ), 4_c_size_t*nrowf)
  d_lev = up(c_loc(lev), 8_c_size_t*nrowf); d_ri = up(c_loc(ri), 8_c_size_t*nrowf); d_rj = up(c_loc(rj), 8_c_size_t*nrowf)
  d_lon = up(c_loc(lon), 8_c_size_t*nrowf); d_lat = up(c_loc(lat), 8_c_size_t*nrowf)
  d_err = up(c_loc(err), 8_c_size_t*nrowf); d_dif = up(c_loc(dif), 8_c_size_t*nrowf)
  d_rotc = up(c_loc(rotc), 16_c_size_t*nrowf); d_own = up(c_loc(own), 4_c_size_t*nrowf)
  dat = 0.0d0                                                        ! obs(iof)%dat = 0.0d0 (obsope_tools.f90:807-809)
  d_dat = up(c_loc(dat), 8_c_size_t*nrowf)
  CALL chk(hipMalloc(d_v3, 8_c_size_t*SIZE(v3)), 'hipMalloc v3d')
  CALL chk(hipMalloc(d_v2, 8_c_size_t*SIZE(v2)), 'hipMalloc v2d')
  CALL chk(hipMalloc(d_counts, 16_c_size_t), 'hipMalloc counts')

  prm%lon = d_lon; prm%lat = d_lat; prm%file_radar = c_loc(file_radar); prm%radar_meta = c_loc(radar_meta)
  prm%rotc = d_rotc; prm%use_obs = c_loc(use_obs)
  prm%nobtype = nobtype; prm%method_ref_calc = h(10); prm%use_terminal_velocity = h(11); prm%stggrd = h(12)
  prm%min_radar_ref_dbz = r(1); prm%low_ref_shift = r(2); prm%radar_zmax = r(3); prm%ps_adjust_thres = r(4)
  prm%ri_off = r(5); prm%rj_off = r(6)
  fl%nlev = nlev; fl%nlon = nlon; fl%nlat = nlat; fl%khalo = khalo; fl%ihalo = ihalo; fl%jhalo = jhalo
  fl%nv3dd = 13; fl%nv2dd = 7; fl%nmem = 1; fl%m0 = 0
  fl%v3d = d_v3; fl%s3k = 1; fl%s3i = nlevh; fl%s3j = INT(nlevh, c_int64_t)*nlonh; fl%s3v = fl%s3j*nlath; fl%s3m = fl%s3v*13
  fl%v2d = d_v2; fl%s2i = 1; fl%s2j = nlonh; fl%s2v = INT(nlonh, c_int64_t)*nlath; fl%s2m = fl%s2v*7
  slot%dif = d_dif; slot%own = MERGE(d_own, c_null_ptr, h(17) /= 0); slot%outside_undef = h(15); slot%reserved0 = 0

  DO islot = 1, nslot
    ! ---- call read_ens_history_iter(1,islot,v3dg,v2dg): the nature run of the slot, here from the case file to the device
    READ (u) v3, v2
    CALL chk(hipMemcpy(d_v3, c_loc(v3), 8_c_size_t*SIZE(v3), hipMemcpyHostToDevice), 'upload v3d')
    CALL chk(hipMemcpy(d_v2, c_loc(v2), 8_c_size_t*SIZE(v2), hipMemcpyHostToDevice), 'upload v2d')
    slot%slot_lb = r(7) + REAL(islot - 1, c_double)*r(8)
    slot%slot_ub = slot%slot_lb + r(8)
    CALL obsmake_slot_amd(ctx, slot, prm, nfile, off, d_elm, d_typ, d_lev, d_ri, d_rj, d_dat, fl, d_counts, ierr)
    CALL chk(INT(ierr, c_int), 'obsmake_slot_amd')
    CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')             ! (the entry is asynchronous: before v3d / v2d are overwritten)
    CALL chk(hipMemcpy(c_loc(counts(1, islot)), d_counts, 16_c_size_t, hipMemcpyDeviceToHost), 'download counts')   ! nslot, nobs_slot
  END DO
  CLOSE (u)
  CALL chk(hipMemcpy(c_loc(dat), d_dat, 8_c_size_t*nrowf, hipMemcpyDeviceToHost), 'download dat')
  OPEN (newunit=uo, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (uo) counts, dat

  ! ---- (MPI_REDUCE of dat over the subdomains: one subdomain here) ; call com_randn(nobsall, error) and the loop at :1006-1049
  IF (seed < 0) THEN
    CALL DATE_AND_TIME(VALUES=idate)
    seed = idate(8) + idate(7)*1000
  END IF
  CALL rand_create_amd(seed, rand, ierr)
  CALL chk(INT(ierr, c_int), 'rand_create_amd')
  errs%obserr_u = oe(1); errs%obserr_v = oe(2); errs%obserr_t = oe(3); errs%obserr_q = oe(4); errs%obserr_rh = oe(5)
  errs%obserr_ps = oe(6); errs%obserr_radar_ref = oe(7); errs%obserr_radar_vr = oe(8)
  CALL obsmake_noise_amd(ctx, errs, nfile, off, d_elm, d_dat, d_err, rand, ierr)
  CALL chk(INT(ierr, c_int), 'obsmake_noise_amd')
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
  CALL chk(hipMemcpy(c_loc(dat), d_dat, 8_c_size_t*nrowf, hipMemcpyDeviceToHost), 'download dat')
  CALL chk(hipMemcpy(c_loc(err), d_err, 8_c_size_t*nrowf, hipMemcpyDeviceToHost), 'download err')
  WRITE (uo) dat, err
  CLOSE (uo)
  rc = letkf_rand_destroy(rand)
  rc = letkf_ctx_destroy(ctx)

CONTAINS

  FUNCTION up(host, nbytes_) RESULT(d)
    TYPE(c_ptr), INTENT(IN) :: host
    INTEGER(c_size_t), INTENT(IN) :: nbytes_
    TYPE(c_ptr) :: d
    CALL chk(hipMalloc(d, MAX(nbytes_, 8_c_size_t)), 'hipMalloc')
    IF (nbytes_ > 0) CALL chk(hipMemcpy(d, host, nbytes_, hipMemcpyHostToDevice), 'hipMemcpy H2D')
  END FUNCTION up

  SUBROUTINE chk(rc_, what)
    INTEGER(c_int), INTENT(IN) :: rc_
    CHARACTER(*), INTENT(IN) :: what
    IF (rc_ /= 0) THEN
      WRITE (6, *) 'error', rc_, 'in ', what
      STOP 5
    END IF
  END SUBROUTINE chk

END PROGRAM obsmake_driver
