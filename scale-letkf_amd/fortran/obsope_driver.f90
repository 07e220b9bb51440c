!===============================================================================
! obsope_driver.f90 -- the chain of three replaced CALLs from a Fortran host:
!   CALL obsope_cal      -> upload of the files, obsda's set / idx and the members' history fields, CALL obsope_amd
!   CALL set_letkf_obs   -> CALL set_letkf_obs_amd with the ensval / qc the operator left (the table stays on the device)
!   CALL das_letkf       -> CALL das_letkf_amd(ctx, nml, tabd, ...) as letkf_analysis_driver.f90 shows it; not repeated here
! Reads a case written by tests/test_fortran_obsope.py and writes ensval / qc as the operator leaves them, then the number of
! rows set_letkf_obs_amd accepted.
!   file layout (little endian, stream):
!     int32 nlev, nlon, nlat, khalo, ihalo, jhalo, nmem, nfile, nrowf, nobs, nobtype, method, use_tv, stggrd, nradar, with_setobs
!     real64 min_radar_ref_dbz, low_ref_shift, radar_zmax, ps_adjust_thres, ri_off, rj_off
!     int64 off(nfile+1) ; int32 file_radar(nfile) ; real64 radar_meta(3,nradar) ; int32 use_obs(nobtype)
!     int32 elm(nrowf), typ(nrowf) ; real64 lev, ri, rj, lon, lat, dat, err (nrowf each)
!     int32 set(nobs), idx(nobs) ; real64 rotc(2,nobs)
!     real64 v3d(nlevh,nlonh,nlath,13,nmem), v2d(nlonh,nlath,7,nmem)      the reference's layout per member
!   with_setobs = 1: the namelist of set_letkf_obs is that of tests/_setobs.py namelist() and tests/_obsprep.py qc_params()
!===============================================================================
PROGRAM obsope_driver
  USE letkf_obsope_amd
  USE letkf_tools_amd
  USE letkf_obs_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: h(16)
  REAL(c_double) :: r(6)
  INTEGER(c_int64_t), ALLOCATABLE, TARGET :: off(:)
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: file_radar(:), use_obs(:), elm(:), typ(:), set(:), idx(:), qc(:)
  REAL(c_double), ALLOCATABLE, TARGET :: radar_meta(:, :), lev(:), ri(:), rj(:), lon(:), lat(:), dat(:), err(:), rotc(:, :), &
                                         v3d(:, :, :, :, :), v2d(:, :, :, :), ensval(:, :)
  INTEGER :: u, ios, nlev, nlon, nlat, khalo, ihalo, jhalo, nmem, nfile, nrowf, nobs, nobtype, nradar, nlevh, nlonh, nlath, ierr
  INTEGER(c_int) :: rc
  TYPE(c_ptr) :: ctx, d_elm, d_typ, d_lev, d_ri, d_rj, d_lon, d_lat, d_set, d_idx, d_rotc, d_v3, d_v2, d_qc, d_ens
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
  nobs = h(10); nobtype = h(11); nradar = h(15)
  nlevh = nlev + 2*khalo; nlonh = nlon + 2*ihalo; nlath = nlat + 2*jhalo
  ALLOCATE (off(nfile + 1), file_radar(nfile), radar_meta(3, MAX(nradar, 1)), use_obs(nobtype), elm(nrowf), typ(nrowf), &
            lev(nrowf), ri(nrowf), rj(nrowf), lon(nrowf), lat(nrowf), dat(nrowf), err(nrowf), set(nobs), idx(nobs), &
            rotc(2, nobs), v3d(nlevh, nlonh, nlath, 13, nmem), v2d(nlonh, nlath, 7, nmem), ensval(nmem, nobs), qc(nobs))
  READ (u) off, file_radar
  IF (nradar > 0) READ (u) radar_meta
  READ (u) use_obs, elm, typ, lev, ri, rj, lon, lat, dat, err, set, idx, rotc, v3d, v2d
  CLOSE (u)

  ! ---- CALL obsope_cal: the files, obsda and the members' fields go to the device once, the operator fills ensval / qc there
  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  d_elm = up(c_loc(elm), 4_c_size_t*nrowf); d_typ = up(c_loc(typ), 4_c_size_t*nrowf)
  d_lev = up(c_loc(lev), 8_c_size_t*nrowf); d_ri = up(c_loc(ri), 8_c_size_t*nrowf); d_rj = up(c_loc(rj), 8_c_size_t*nrowf)
  d_lon = up(c_loc(lon), 8_c_size_t*nrowf); d_lat = up(c_loc(lat), 8_c_size_t*nrowf)
  d_set = up(c_loc(set), 4_c_size_t*nobs); d_idx = up(c_loc(idx), 4_c_size_t*nobs)
  d_rotc = up(c_loc(rotc), 16_c_size_t*nobs)
  d_v3 = up(c_loc(v3d), 8_c_size_t*SIZE(v3d)); d_v2 = up(c_loc(v2d), 8_c_size_t*SIZE(v2d))
  qc = 0; ensval = 0.0d0
  d_qc = up(c_loc(qc), 4_c_size_t*nobs); d_ens = up(c_loc(ensval), 8_c_size_t*nmem*nobs)

  prm%lon = d_lon; prm%lat = d_lat; prm%file_radar = c_loc(file_radar); prm%radar_meta = c_loc(radar_meta)
  prm%rotc = d_rotc; prm%use_obs = c_loc(use_obs)
  prm%nobtype = nobtype; prm%method_ref_calc = h(12); prm%use_terminal_velocity = h(13); prm%stggrd = h(14)
  prm%min_radar_ref_dbz = r(1); prm%low_ref_shift = r(2); prm%radar_zmax = r(3); prm%ps_adjust_thres = r(4)
  prm%ri_off = r(5); prm%rj_off = r(6)
  fl%nlev = nlev; fl%nlon = nlon; fl%nlat = nlat; fl%khalo = khalo; fl%ihalo = ihalo; fl%jhalo = jhalo
  fl%nv3dd = 13; fl%nv2dd = 7; fl%nmem = nmem; fl%m0 = 0
  fl%v3d = d_v3; fl%s3k = 1; fl%s3i = nlevh; fl%s3j = INT(nlevh, c_int64_t)*nlonh; fl%s3v = fl%s3j*nlath; fl%s3m = fl%s3v*13
  fl%v2d = d_v2; fl%s2i = 1; fl%s2j = nlonh; fl%s2v = INT(nlonh, c_int64_t)*nlath; fl%s2m = fl%s2v*7
  CALL obsope_amd(ctx, prm, nfile, off, d_elm, d_typ, d_lev, d_ri, d_rj, fl, 1_c_int64_t, INT(nobs, c_int64_t), d_set, d_idx, &
                  d_qc, d_ens, INT(nmem, c_int64_t), ierr)
  CALL chk(INT(ierr, c_int), 'obsope_amd')
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
  CALL chk(hipMemcpy(c_loc(ensval), d_ens, 8_c_size_t*nmem*nobs, hipMemcpyDeviceToHost), 'download ensval')
  CALL chk(hipMemcpy(c_loc(qc), d_qc, 4_c_size_t*nobs, hipMemcpyDeviceToHost), 'download qc')
  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) ensval, qc

  ! ---- CALL set_letkf_obs: obsda as the operator left it; the files are pre-processed only now
  IF (h(16) /= 0) THEN
    onml%nobtype = nobtype; onml%nlon = nlon; onml%nlat = nlat; onml%ihalo = ihalo; onml%jhalo = jhalo
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
    CALL set_letkf_obs_amd(ctx, onml, nfile, off, elm, typ, lev, dat, err, ri, rj, nobs, set, idx, qc, ensval, tabd)
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

END PROGRAM obsope_driver
