!===============================================================================
! obsscan_driver.f90 -- CALL obsope_cal replaced whole from a Fortran host, then CALL set_letkf_obs:
!   first scan + bucket sort  -> upload of ri / rj / dif, CALL obsscan_amd: obsda's set / idx / qc on the device, bsn / bsna here
!   second scan               -> per subdomain and time slot CALL obsope_slot_amd with that subdomain's history fields
!   CALL set_letkf_obs        -> CALL set_letkf_obs_amd with the lists, ensval and qc as they stand
! (obsope_driver.f90 is the same chain with obsda's rows made by hand.)  Reads a case written by tests/test_fortran_obsscan.py
! and writes bsn, bsna, set, idx, qc and ensval, then the number of rows set_letkf_obs_amd accepted.
!   file layout (little endian, stream):
!     int32 nlev, nlon, nlat, khalo, ihalo, jhalo, nmem, nfile, nrowf, nlist, nobtype, method, use_tv, stggrd, nradar, with_setobs,
!           prc_num_x, prc_num_y, slot_start, slot_end, slot_base                 (nlon, nlat: of one subdomain)
!     real64 min_radar_ref_dbz, low_ref_shift, radar_zmax, ps_adjust_thres, slot_tinterval
!     int64 off(nfile+1) ; int32 file_radar(nfile), obsda_run(nfile) ; real64 radar_meta(3,nradar) ; int32 use_obs(nobtype)
!     int32 elm(nrowf), typ(nrowf) ; real64 lev, ri, rj, lon, lat, dat, err, dif (nrowf each)
!     real64 v3d(nlevh,nlonh,nlath,13,nmem,nprocs_d), v2d(nlonh,nlath,7,nmem,nprocs_d)      the reference's layout per subdomain
!   with_setobs = 1: the namelist of set_letkf_obs is obsope_driver.f90's, on the whole domain
!===============================================================================
PROGRAM obsscan_driver
  USE letkf_obsscan_amd
  USE letkf_tools_amd
  USE letkf_obs_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: h(21)
  REAL(c_double) :: r(5)
  INTEGER(c_int64_t), ALLOCATABLE, TARGET :: off(:)
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: file_radar(:), obsda_run(:), use_obs(:), elm(:), typ(:), set(:), idx(:), qc(:), &
                                             bsn(:, :), bsna(:, :)
  REAL(c_double), ALLOCATABLE, TARGET :: radar_meta(:, :), lev(:), ri(:), rj(:), lon(:), lat(:), dat(:), err(:), dif(:), &
                                         rotc(:, :), v3d(:, :, :, :, :, :), v2d(:, :, :, :, :), ensval(:, :)
  INTEGER :: u, ios, nlev, nlon, nlat, khalo, ihalo, jhalo, nmem, nfile, nrowf, nlist, nobtype, nradar, nlevh, nlonh, nlath, ierr
  INTEGER :: px, py, nprocs, s0, s1, ip, islot
  INTEGER(c_int) :: rc
  TYPE(c_ptr) :: ctx, d_elm, d_typ, d_lev, d_ri, d_rj, d_lon, d_lat, d_dif, d_set, d_idx, d_rotc, d_qc, d_ens
  TYPE(c_ptr), ALLOCATABLE :: d_v3(:), d_v2(:)
  TYPE(letkf_obsscan_params) :: sp
  TYPE(letkf_obsscan_lists) :: lists
  TYPE(letkf_obsope_params) :: prm
  TYPE(letkf_obsope_fields) :: fl
  TYPE(letkf_obs_nml) :: onml
  TYPE(letkf_obs_tables_dev) :: tabd
  CHARACTER(len=512) :: fin, fout

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) h
  READ (u) r
  nlev = h(1); nlon = h(2); nlat = h(3); khalo = h(4); ihalo = h(5); jhalo = h(6); nmem = h(7); nfile = h(8); nrowf = h(9)
  nlist = h(10); nobtype = h(11); nradar = h(15); px = h(17); py = h(18); s0 = h(19); s1 = h(20)
  nprocs = px*py
  nlevh = nlev + 2*khalo; nlonh = nlon + 2*ihalo; nlath = nlat + 2*jhalo
  ALLOCATE (off(nfile + 1), file_radar(nfile), obsda_run(nfile), radar_meta(3, MAX(nradar, 1)), use_obs(nobtype), elm(nrowf), &
            typ(nrowf), lev(nrowf), ri(nrowf), rj(nrowf), lon(nrowf), lat(nrowf), dat(nrowf), err(nrowf), dif(nrowf), &
            set(nlist), idx(nlist), qc(nlist), rotc(2, nlist), ensval(nmem, nlist), &
            v3d(nlevh, nlonh, nlath, 13, nmem, nprocs), v2d(nlonh, nlath, 7, nmem, nprocs), &
            bsn(s0:s1 + 2, 0:nprocs - 1), bsna(s0 - 1:s1 + 2, 0:nprocs - 1), d_v3(0:nprocs - 1), d_v2(0:nprocs - 1))
  READ (u) off, file_radar, obsda_run
  IF (nradar > 0) READ (u) radar_meta
  READ (u) use_obs, elm, typ, lev, ri, rj, lon, lat, dat, err, dif, v3d, v2d
  CLOSE (u)

  ! ---- the first scan: the files' coordinates and time differences go to the device once, the lists stay there
  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  d_elm = up(c_loc(elm), 4_c_size_t*nrowf); d_typ = up(c_loc(typ), 4_c_size_t*nrowf)
  d_lev = up(c_loc(lev), 8_c_size_t*nrowf); d_ri = up(c_loc(ri), 8_c_size_t*nrowf); d_rj = up(c_loc(rj), 8_c_size_t*nrowf)
  d_lon = up(c_loc(lon), 8_c_size_t*nrowf); d_lat = up(c_loc(lat), 8_c_size_t*nrowf); d_dif = up(c_loc(dif), 8_c_size_t*nrowf)
  set = 0; idx = 0; qc = 0; ensval = 0.0d0; rotc(1, :) = 1.0d0; rotc(2, :) = 0.0d0
  d_set = up(c_loc(set), 4_c_size_t*nlist); d_idx = up(c_loc(idx), 4_c_size_t*nlist); d_qc = up(c_loc(qc), 4_c_size_t*nlist)
  d_rotc = up(c_loc(rotc), 16_c_size_t*nlist); d_ens = up(c_loc(ensval), 8_c_size_t*nmem*nlist)
  sp%obsda_run = c_loc(obsda_run)
  sp%nlon = nlon; sp%nlat = nlat; sp%ihalo = ihalo; sp%jhalo = jhalo; sp%prc_num_x = px; sp%prc_num_y = py
  sp%slot_start = s0; sp%slot_end = s1; sp%slot_base = h(21); sp%myrank_d = 0; sp%slot_tinterval = r(5)
  CALL obsscan_amd(ctx, sp, nfile, off, d_ri, d_rj, d_dif, d_set, d_idx, d_qc, bsn, bsna, ierr)
  CALL chk(INT(ierr, c_int), 'obsscan_amd')

  ! ---- the second scan: one call per subdomain and time slot, each with the fields the host holds for it
  lists%nprocs_d = nprocs; lists%slot_start = s0; lists%slot_end = s1; lists%reserved0 = 0
  lists%bsna = c_loc(bsna); lists%set = d_set; lists%idx = d_idx; lists%qc = d_qc
  prm%lon = d_lon; prm%lat = d_lat; prm%file_radar = c_loc(file_radar); prm%radar_meta = c_loc(radar_meta)
  prm%rotc = d_rotc; prm%use_obs = c_loc(use_obs)
  prm%nobtype = nobtype; prm%method_ref_calc = h(12); prm%use_terminal_velocity = h(13); prm%stggrd = h(14)
  prm%min_radar_ref_dbz = r(1); prm%low_ref_shift = r(2); prm%radar_zmax = r(3); prm%ps_adjust_thres = r(4)
  fl%nlev = nlev; fl%nlon = nlon; fl%nlat = nlat; fl%khalo = khalo; fl%ihalo = ihalo; fl%jhalo = jhalo
  fl%nv3dd = 13; fl%nv2dd = 7; fl%nmem = nmem; fl%m0 = 0
  fl%s3k = 1; fl%s3i = nlevh; fl%s3j = INT(nlevh, c_int64_t)*nlonh; fl%s3v = fl%s3j*nlath; fl%s3m = fl%s3v*13
  fl%s2i = 1; fl%s2j = nlonh; fl%s2v = INT(nlonh, c_int64_t)*nlath; fl%s2m = fl%s2v*7
  DO ip = 0, nprocs - 1
    d_v3(ip) = up(c_loc(v3d(1, 1, 1, 1, 1, ip + 1)), 8_c_size_t*SIZE(v3d)/nprocs)
    d_v2(ip) = up(c_loc(v2d(1, 1, 1, 1, ip + 1)), 8_c_size_t*SIZE(v2d)/nprocs)
    prm%ri_off = REAL(MOD(ip, px)*nlon, c_double); prm%rj_off = REAL((ip/px)*nlat, c_double)       ! rij_g2l
    fl%v3d = d_v3(ip); fl%v2d = d_v2(ip)
    DO islot = s0, s1
      IF (bsn(islot, ip) == 0) CYCLE                                   ! (the host would not read this slot's fields)
      CALL obsope_slot_amd(ctx, lists, ip, islot, prm, nfile, off, d_elm, d_typ, d_lev, d_ri, d_rj, fl, d_ens, &
                           INT(nmem, c_int64_t), ierr)
      CALL chk(INT(ierr, c_int), 'obsope_slot_amd')
    END DO
  END DO
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
  CALL chk(hipMemcpy(c_loc(set), d_set, 4_c_size_t*nlist, hipMemcpyDeviceToHost), 'download set')
  CALL chk(hipMemcpy(c_loc(idx), d_idx, 4_c_size_t*nlist, hipMemcpyDeviceToHost), 'download idx')
  CALL chk(hipMemcpy(c_loc(qc), d_qc, 4_c_size_t*nlist, hipMemcpyDeviceToHost), 'download qc')
  CALL chk(hipMemcpy(c_loc(ensval), d_ens, 8_c_size_t*nmem*nlist, hipMemcpyDeviceToHost), 'download ensval')
  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) bsn, bsna, set, idx, qc, ensval

  ! ---- CALL set_letkf_obs: obsda as the two scans left it
  IF (h(16) /= 0) THEN
    onml%nobtype = nobtype; onml%nlon = nlon*px; onml%nlat = nlat*py; onml%ihalo = ihalo; onml%jhalo = jhalo
    ALLOCATE (onml%hori_local(nobtype), onml%vert_local(nobtype), onml%obs_sort_grid_spacing(nobtype), &
              onml%obs_min_spacing(nobtype), onml%max_nobs_per_grid(nobtype))
    onml%hori_local = 3000.0d0; onml%hori_local(1) = 4000.0d0; onml%hori_local(8) = 5000.0d0
    onml%hori_local(22) = 2500.0d0; onml%hori_local(23) = 3500.0d0
    onml%vert_local = 0.4d0; onml%vert_local(22) = 3000.0d0
    onml%obs_sort_grid_spacing = 0.0d0; onml%obs_sort_grid_spacing(8) = 3000.0d0
    onml%max_nobs_per_grid = 0; onml%max_nobs_per_grid(22) = 40
    onml%obs_min_spacing = 300.0d0
    onml%min_radar_ref_dbz = r(1); onml%low_ref_shift = r(2)
    onml%use_obserr_radar_ref = .TRUE.; onml%obserr_radar_ref = 5.0d0; onml%use_obserr_radar_vr = .TRUE.; onml%obserr_radar_vr = 3.0d0
    onml%hori_local_radar_obsnoref = 2000.0d0; onml%hori_local_radar_vr = 2200.0d0; onml%vert_local_radar_vr = 2500.0d0
    onml%dx = 1000.0d0; onml%dy = 1000.0d0; onml%vert_local_rain_base = 85000.0d0; onml%max_nobs_per_grid_criterion = 1
    onml%log_level = 0
    onml%qc%member = nmem; onml%qc%det_run = 0; onml%qc%use_radar_ref = 1; onml%qc%use_radar_vr = 1
    onml%qc%min_radar_ref_member = 3; onml%qc%min_radar_ref_member_obsref = 2; onml%qc%radar_ref_thres_dbz = 15.0d0
    onml%qc%gross_error = 5.0d0; onml%qc%gross_error_rain = 4.0d0; onml%qc%gross_error_radar_ref = 3.0d0
    onml%qc%gross_error_radar_vr = 2.5d0; onml%qc%gross_error_radar_prh = 5.0d0; onml%qc%gross_error_tcx = 5.0d0
    onml%qc%gross_error_tcy = 5.0d0; onml%qc%gross_error_tcp = 5.0d0
    onml%qc%h08 = 0; onml%qc%h08_min_cld_member = 0; onml%qc%h08_limit_lev = 0.0d0; onml%qc%gross_error_h08 = 0.0d0
    onml%qc%h08_bt_min = 0.0d0; onml%qc%h08_lev = c_null_ptr; onml%qc%h08_val2 = c_null_ptr
    CALL set_letkf_obs_amd(ctx, onml, nfile, off, elm, typ, lev, dat, err, ri, rj, nlist, set, idx, qc, ensval, tabd)
    WRITE (u) INT(tabd%host%nobstotal, c_int32_t)
    CALL letkf_obs_tables_dev_free(tabd)
  END IF
  CLOSE (u)
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

END PROGRAM obsscan_driver
