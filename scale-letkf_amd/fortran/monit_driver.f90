!===============================================================================
! monit_driver.f90 -- the departure monitor from a Fortran host: what write_ensmean(..., monit_step=1) and
! write_ens_mpi(..., monit_step=2) do with the guess mean and the analysis mean under DEPARTURE_STAT, with the states on the
! device:  CALL state_to_history_amd + CALL monit_obs_amd at step 1 on one state and at step 2 on a second, CALL
! monit_print_amd after each.  Reads a case written by tests/test_fortran_monit.py, prints both tables, writes the records
! and the statistics after each step.
!   file layout (little endian, stream):
!     int32 nlev, nlon, nlat, khalo, ihalo, jhalo, nfile, nrowf, nobs, nobtype, method, use_tv, stggrd, nradar, nv3d, edge_fill,
!           departure_stat_radar, nkey (-1: no key), 0, 0
!     real64 min_radar_ref_dbz, low_ref_shift, radar_zmax, ps_adjust_thres, ri_off, rj_off, t_range, ztop
!     int64 off(nfile+1) ; int32 file_radar(nfile) ; real64 radar_meta(3,nradar) ; int32 use_obs(nobtype)
!     int32 elm(nrowf), typ(nrowf) ; real64 lev, ri, rj, lon, lat, dat, dif (nrowf each)
!     int32 set(nobs), idx(nobs) ; real64 rotc(2,nobs) ; int32 key(nkey), 0-based
!     real64 cz(nlev), topo(nlon,nlat), gues(nlon,nlat,nlev,nv3d), anal(nlon,nlat,nlev,nv3d)      point-fastest states
!   output: per step  int32 set(nn), idx(nn), qc(nn) ; real64 omb(nn), oma(nn) ; int32 nobs(16) ; real64 bias(16), rmse(16)
!===============================================================================
PROGRAM monit_driver
  USE letkf_monit_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: h(20)
  REAL(c_double) :: r(8)
  INTEGER(c_int64_t), ALLOCATABLE, TARGET :: off(:)
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: file_radar(:), use_obs(:), elm(:), typ(:), set(:), idx(:), key(:), rset(:), ridx(:), rqc(:)
  REAL(c_double), ALLOCATABLE, TARGET :: radar_meta(:, :), lev(:), ri(:), rj(:), lon(:), lat(:), dat(:), dif(:), rotc(:, :), &
                                         cz(:), topo(:, :), xs(:, :, :, :, :), romb(:), roma(:)
  INTEGER(c_int32_t), TARGET :: uid(nid_obs_monit), nobs(nid_obs_monit)
  REAL(c_double), TARGET :: bias(nid_obs_monit), rmse(nid_obs_monit)
  LOGICAL :: mtype(nid_obs_monit)
  INTEGER :: u, uo, ios, nlev, nlon, nlat, khalo, ihalo, jhalo, nfile, nrowf, nobs_da, nobtype, nradar, nv3d, nkey, nlevh, nlonh, &
             nlath, ierr, step
  INTEGER(c_int64_t) :: nn
  INTEGER(c_int) :: rc
  TYPE(c_ptr) :: ctx, d_elm, d_typ, d_lev, d_ri, d_rj, d_lon, d_lat, d_dat, d_dif, d_set, d_idx, d_rotc, d_key, d_topo, d_x(2), &
                 d_v3, d_v2
  TYPE(letkf_obsope_params) :: prm
  TYPE(letkf_obsope_fields) :: fl
  TYPE(letkf_hist_state) :: st
  TYPE(letkf_monit_params) :: mprm
  TYPE(letkf_obsdep) :: rec
  CHARACTER(len=512) :: fin, fout

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) h
  READ (u) r
  nlev = h(1); nlon = h(2); nlat = h(3); khalo = h(4); ihalo = h(5); jhalo = h(6); nfile = h(7); nrowf = h(8); nobs_da = h(9)
  nobtype = h(10); nradar = h(14); nv3d = h(15); nkey = h(18)
  nlevh = nlev + 2*khalo; nlonh = nlon + 2*ihalo; nlath = nlat + 2*jhalo
  nn = MERGE(nkey, nobs_da, nkey >= 0)
  ALLOCATE (off(nfile + 1), file_radar(nfile), radar_meta(3, MAX(nradar, 1)), use_obs(nobtype), elm(nrowf), typ(nrowf), &
            lev(nrowf), ri(nrowf), rj(nrowf), lon(nrowf), lat(nrowf), dat(nrowf), dif(nrowf), set(nobs_da), idx(nobs_da), &
            rotc(2, nobs_da), key(MAX(nkey, 1)), cz(nlev), topo(nlon, nlat), xs(nlon, nlat, nlev, nv3d, 2), &
            rset(MAX(nn, 1)), ridx(MAX(nn, 1)), rqc(MAX(nn, 1)), romb(MAX(nn, 1)), roma(MAX(nn, 1)))
  key = 0; rset = 0; ridx = 0; rqc = 0; romb = 0.0d0; roma = 0.0d0
  READ (u) off, file_radar
  IF (nradar > 0) READ (u) radar_meta
  READ (u) use_obs, elm, typ, lev, ri, rj, lon, lat, dat, dif, set, idx, rotc
  IF (nkey > 0) READ (u) key(1:nkey)
  READ (u) cz, topo, xs
  CLOSE (u)

  ! ---- the files as set_letkf_obs left them, obsda's set / idx (and key) and the two mean states go to the device once
  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  d_elm = up(c_loc(elm), 4_c_size_t*nrowf); d_typ = up(c_loc(typ), 4_c_size_t*nrowf)
  d_lev = up(c_loc(lev), 8_c_size_t*nrowf); d_ri = up(c_loc(ri), 8_c_size_t*nrowf); d_rj = up(c_loc(rj), 8_c_size_t*nrowf)
  d_lon = up(c_loc(lon), 8_c_size_t*nrowf); d_lat = up(c_loc(lat), 8_c_size_t*nrowf)
  d_dat = up(c_loc(dat), 8_c_size_t*nrowf); d_dif = up(c_loc(dif), 8_c_size_t*nrowf)
  d_set = up(c_loc(set), 4_c_size_t*nobs_da); d_idx = up(c_loc(idx), 4_c_size_t*nobs_da)
  d_rotc = up(c_loc(rotc), 16_c_size_t*nobs_da)
  d_key = c_null_ptr
  IF (nkey >= 0) d_key = up(c_loc(key), 4_c_size_t*nkey)
  d_topo = up(c_loc(topo), 8_c_size_t*SIZE(topo))
  d_x(1) = up(c_loc(xs(1, 1, 1, 1, 1)), 8_c_size_t*(SIZE(xs)/2)); d_x(2) = up(c_loc(xs(1, 1, 1, 1, 2)), 8_c_size_t*(SIZE(xs)/2))
  CALL chk(hipMalloc(d_v3, 8_c_size_t*nlevh*nlonh*nlath*13), 'hipMalloc v3d')
  CALL chk(hipMalloc(d_v2, 8_c_size_t*nlonh*nlath*7), 'hipMalloc v2d')
  rec%set = up(c_loc(rset), 4_c_size_t*nn); rec%idx = up(c_loc(ridx), 4_c_size_t*nn); rec%qc = up(c_loc(rqc), 4_c_size_t*nn)
  rec%omb = up(c_loc(romb), 8_c_size_t*nn); rec%oma = up(c_loc(roma), 8_c_size_t*nn)

  prm%lon = d_lon; prm%lat = d_lat; prm%file_radar = c_loc(file_radar); prm%radar_meta = c_loc(radar_meta)
  prm%rotc = d_rotc; prm%use_obs = c_loc(use_obs)
  prm%nobtype = nobtype; prm%method_ref_calc = h(11); prm%use_terminal_velocity = h(12); prm%stggrd = h(13)
  prm%min_radar_ref_dbz = r(1); prm%low_ref_shift = r(2); prm%radar_zmax = r(3); prm%ps_adjust_thres = r(4)
  prm%ri_off = r(5); prm%rj_off = r(6)
  fl%nlev = nlev; fl%nlon = nlon; fl%nlat = nlat; fl%khalo = khalo; fl%ihalo = ihalo; fl%jhalo = jhalo
  fl%nv3dd = 13; fl%nv2dd = 7; fl%nmem = 1; fl%m0 = 0
  fl%v3d = d_v3; fl%s3k = 1; fl%s3i = nlevh; fl%s3j = INT(nlevh, c_int64_t)*nlonh; fl%s3v = fl%s3j*nlath; fl%s3m = fl%s3v*13
  fl%v2d = d_v2; fl%s2i = 1; fl%s2j = nlonh; fl%s2v = INT(nlonh, c_int64_t)*nlath; fl%s2m = fl%s2v*7
  st%nv3d = nv3d; st%edge_fill = h(16)
  st%si = 1; st%sj = nlon; st%sl = INT(nlon, c_int64_t)*nlat; st%sv = st%sl*nlev
  st%topo = d_topo; st%cz = c_loc(cz); st%ztop = r(8)
  uid = elem_uid_monit
  mprm%departure_stat_radar = h(17); mprm%nid = nid_obs_monit; mprm%reserved0 = 0
  mprm%elem_uid = c_loc(uid); mprm%t_range = r(7); mprm%dif = d_dif

  OPEN (newunit=uo, file=trim(fout), access='stream', form='unformatted', status='replace')
  DO step = 1, 2
    ! ---- CALL monit_obs(v3dg, v2dg, topo, nobs, bias, rmse, monit_type, use_key, step) on the mean state of this step
    st%x = d_x(step)
    mprm%step = step
    CALL state_to_history_amd(ctx, st, fl, d_v3, d_v2, ierr)
    CALL chk(INT(ierr, c_int), 'state_to_history_amd')
    CALL monit_obs_amd(ctx, mprm, prm, nfile, off, d_elm, d_typ, d_lev, d_ri, d_rj, d_dat, fl, nn, d_key, d_set, d_idx, rec, &
                       nobs, bias, rmse, mtype, ierr)
    CALL chk(INT(ierr, c_int), 'monit_obs_amd')
    CALL monit_print_amd(nobs, bias, rmse, mtype)
    CALL chk(hipMemcpy(c_loc(rset), rec%set, 4_c_size_t*nn, hipMemcpyDeviceToHost), 'download set')
    CALL chk(hipMemcpy(c_loc(ridx), rec%idx, 4_c_size_t*nn, hipMemcpyDeviceToHost), 'download idx')
    CALL chk(hipMemcpy(c_loc(rqc), rec%qc, 4_c_size_t*nn, hipMemcpyDeviceToHost), 'download qc')
    CALL chk(hipMemcpy(c_loc(romb), rec%omb, 8_c_size_t*nn, hipMemcpyDeviceToHost), 'download omb')
    CALL chk(hipMemcpy(c_loc(roma), rec%oma, 8_c_size_t*nn, hipMemcpyDeviceToHost), 'download oma')
    WRITE (uo) rset(1:nn), ridx(1:nn), rqc(1:nn), romb(1:nn), roma(1:nn), nobs, bias, rmse
  END DO
  CLOSE (uo)
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

END PROGRAM monit_driver
