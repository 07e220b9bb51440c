!===============================================================================
! letkf_analysis_driver.f90 -- a Fortran host running the analysis step of PROGRAM letkf (scale/letkf/letkf.f90) on the device:
!   :142  CALL set_letkf_obs_amd   (letkf_obs_amd.f90: the observation table stays on the device)
!   :196  CALL das_letkf_amd       (letkf_tools_amd.f90, the device-table specific: no upload)
!   :207  the analysis mean        (inside das_letkf_amd)
! For comparison it then runs the host-table das_letkf_amd on the same tables, downloaded (letkf_obs_table_download), from
! the same first guess.  Reads a case file written by tests/test_fortran_analysis.py, writes the results.
!   file (little endian, stream): the header and arrays in the order read below
!===============================================================================
PROGRAM letkf_analysis_driver
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_tools_amd
  USE letkf_obs_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: hdr(16), qi(8)
  REAL(c_double) :: r(11), qd(12)
  INTEGER :: member, det, nlon, nlat, nlev, nv3d, nfile, nrows, nobs, kld, nens, nij1, npts, nt, nc, u, ios
  TYPE(letkf_obs_nml) :: onml
  TYPE(letkf_das_nml) :: nml
  TYPE(letkf_obs_tables_dev) :: tabd
  TYPE(letkf_obs_tables), TARGET :: obs
  TYPE(letkf_obs_table_info) :: ti
  TYPE(c_ptr) :: ctx
  INTEGER(c_int64_t), ALLOCATABLE :: off(:)
  INTEGER(c_int32_t), ALLOCATABLE :: elm(:), typ(:), set(:), idx(:), qc(:), np_dev(:, :), np_host(:, :)
  REAL(c_double), ALLOCATABLE :: lev(:), dat(:), err(:), ri(:), rj(:), ensval(:, :), olev(:), val2(:)
  REAL(c_double), ALLOCATABLE :: rig1(:), rjg1(:), hgt1(:, :), gues0(:, :, :, :), gues3d(:, :, :, :), anal_dev(:, :, :, :), &
                                 anal_host(:, :, :, :)
  INTEGER :: mn(16)
  REAL(c_double) :: mb(16), mr(16)
  INTEGER(c_int32_t), POINTER :: ip(:)
  INTEGER(c_int64_t), POINTER :: lp(:)
  CHARACTER(len=512) :: fin, fout
  INTEGER(c_int) :: rc

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) hdr
  member = hdr(1); det = hdr(2); nlon = hdr(3); nlat = hdr(4); nlev = hdr(5); nv3d = hdr(6)
  nfile = hdr(8); nrows = hdr(9); nobs = hdr(10); kld = hdr(11)
  nens = member + 1 + det; nij1 = nlon*nlat; npts = nij1*nlev
  READ (u) r
  ! ---- the namelist of set_letkf_obs
  onml%nlon = nlon; onml%nlat = nlat; onml%ihalo = hdr(7); onml%jhalo = hdr(7)
  onml%use_obserr_radar_ref = hdr(13) /= 0; onml%use_obserr_radar_vr = hdr(14) /= 0
  onml%max_nobs_per_grid_criterion = hdr(15); onml%log_level = hdr(16)
  onml%dx = r(1); onml%dy = r(1); onml%min_radar_ref_dbz = r(2); onml%low_ref_shift = r(3)
  onml%obserr_radar_ref = r(4); onml%obserr_radar_vr = r(5); onml%hori_local_radar_obsnoref = r(6)
  onml%hori_local_radar_vr = r(7); onml%vert_local_radar_vr = r(8); onml%vert_local_rain_base = r(9)
  ALLOCATE (onml%hori_local(24), onml%vert_local(24), onml%obs_sort_grid_spacing(24), onml%obs_min_spacing(24), &
            onml%max_nobs_per_grid(24))
  READ (u) onml%hori_local, onml%vert_local, onml%obs_sort_grid_spacing, onml%obs_min_spacing
  ALLOCATE (ip(24))
  READ (u) ip
  onml%max_nobs_per_grid = ip
  DEALLOCATE (ip)
  READ (u) qi, qd
  onml%qc%member = qi(1); onml%qc%det_run = qi(2); onml%qc%use_radar_ref = qi(3); onml%qc%use_radar_vr = qi(4)
  onml%qc%min_radar_ref_member = qi(5); onml%qc%min_radar_ref_member_obsref = qi(6)
  onml%qc%h08 = qi(7); onml%qc%h08_min_cld_member = qi(8)
  onml%qc%radar_ref_thres_dbz = qd(1); onml%qc%gross_error = qd(2); onml%qc%gross_error_rain = qd(3)
  onml%qc%gross_error_radar_ref = qd(4); onml%qc%gross_error_radar_vr = qd(5); onml%qc%gross_error_radar_prh = qd(6)
  onml%qc%gross_error_tcx = qd(7); onml%qc%gross_error_tcy = qd(8); onml%qc%gross_error_tcp = qd(9)
  onml%qc%h08_limit_lev = qd(10); onml%qc%gross_error_h08 = qd(11); onml%qc%h08_bt_min = qd(12)
  ! ---- the observation files (read_obs_all) and obsda (obsope)
  ALLOCATE (off(nfile + 1), elm(nrows), typ(nrows), lev(nrows), dat(nrows), err(nrows), ri(nrows), rj(nrows))
  READ (u) off, elm, typ, lev, dat, err, ri, rj
  ALLOCATE (set(nobs), idx(nobs), qc(nobs), ensval(kld, nobs), olev(nobs), val2(nobs))
  READ (u) set, idx, qc, ensval, olev, val2
  ! ---- das_letkf's namelist, the grid and the first guess
  nml%member = member; nml%det_run = det /= 0
  nml%relax_alpha_spread = r(10); nml%infl_mul = r(11); nml%infl_mul_min = -1.0d0
  nml%max_nobs_per_grid_criterion = hdr(15); nml%vert_local_rain_base = r(9)
  nml%dx = r(1); nml%dy = r(1); nml%ihalo = hdr(7); nml%jhalo = hdr(7); nml%nlon = nlon; nml%nlat = nlat
  nml%nlong = nlon; nml%nlatg = nlat; nml%i_org = hdr(7) + 0.5d0; nml%j_org = hdr(7) + 0.5d0
  nml%vert_local_radar = MAX(onml%vert_local(22), onml%vert_local_radar_vr); nml%radar_zmax = 99.0d3
  nml%iv3d_p = 5; nml%iv3d_q = 6; nml%iv3d_qlast = MIN(11, nv3d)
  ALLOCATE (nml%var_local(nv3d, 9), nml%ctype_merge(16, 24))
  READ (u) nml%var_local
  nml%ctype_merge = 0
  ALLOCATE (rig1(nij1), rjg1(nij1), hgt1(nij1, nlev), gues0(nij1, nlev, nens, nv3d))
  READ (u) rig1, rjg1, hgt1, gues0
  CLOSE (u)

  IF (letkf_amd_abi_version() < 8) STOP 4
  rc = letkf_ctx_create(0_c_int, ctx)
  IF (rc /= 0) STOP 5
  ALLOCATE (gues3d(nij1, nlev, nens, nv3d), anal_dev(nij1, nlev, nens, nv3d), anal_host(nij1, nlev, nens, nv3d), &
            np_dev(nij1, nlev), np_host(nij1, nlev))

  ! ---- letkf.f90:142 -> 196 -> 207 with the table on the device
  IF (hdr(12) /= 0) THEN
    CALL set_letkf_obs_amd(ctx, onml, nfile, off, elm, typ, lev, dat, err, ri, rj, nobs, set, idx, qc, ensval, tabd, &
                           obsda_lev=olev, obsda_val2=val2, monit_nobs=mn, monit_bias=mb, monit_rmse=mr)
  ELSE
    CALL set_letkf_obs_amd(ctx, onml, nfile, off, elm, typ, lev, dat, err, ri, rj, nobs, set, idx, qc, ensval, tabd, &
                           monit_nobs=mn, monit_bias=mb, monit_rmse=mr)
  END IF
  gues3d = gues0
  CALL das_letkf_amd(ctx, nml, tabd, nij1, nlev, nens, nv3d, rig1, rjg1, hgt1, gues3d, anal_dev, nobs_point=np_dev)

  ! ---- the same analysis from the host-table specific on the downloaded tables
  obs = tabd%host
  nt = obs%nobstotal; nc = obs%nctype
  rc = letkf_obs_table_info_get(tabd%handle, ti)
  ALLOCATE (obs%ngrd_i(nc), obs%ngrd_j(nc), obs%ngrdsch_i(nc), obs%ngrdsch_j(nc), obs%ngrdext_i(nc), obs%ngrdext_j(nc), &
            obs%ac_off(nc), obs%ac_ext(MAX(ti%nacx, 1_c_int64_t)), obs%ob_ri(MAX(nt, 1)), obs%ob_rj(MAX(nt, 1)), &
            obs%ob_lev(MAX(nt, 1)), obs%ob_dat(MAX(nt, 1)), obs%ob_err(MAX(nt, 1)), obs%ensval(kld, MAX(nt, 1)), obs%val(MAX(nt, 1)))
  CALL c_f_pointer(ti%ngrd_i, ip, (/nc/)); obs%ngrd_i = ip
  CALL c_f_pointer(ti%ngrd_j, ip, (/nc/)); obs%ngrd_j = ip
  CALL c_f_pointer(ti%ngrdsch_i, ip, (/nc/)); obs%ngrdsch_i = ip
  CALL c_f_pointer(ti%ngrdsch_j, ip, (/nc/)); obs%ngrdsch_j = ip
  CALL c_f_pointer(ti%ngrdext_i, ip, (/nc/)); obs%ngrdext_i = ip
  CALL c_f_pointer(ti%ngrdext_j, ip, (/nc/)); obs%ngrdext_j = ip
  CALL c_f_pointer(ti%ac_off, lp, (/nc/)); obs%ac_off = lp
  rc = letkf_obs_table_download(ctx, tabd%handle, c_loc(obs%ensval), c_loc(obs%val), c_null_ptr, c_loc(obs%ob_ri), &
                                c_loc(obs%ob_rj), c_loc(obs%ob_lev), c_loc(obs%ob_dat), c_loc(obs%ob_err), c_loc(obs%ac_ext))
  IF (rc /= 0) STOP 6
  gues3d = gues0
  CALL das_letkf_amd(ctx, nml, obs, nij1, nlev, nens, nv3d, rig1, rjg1, hgt1, gues3d, anal_host, nobs_point=np_host)
  CALL letkf_obs_tables_dev_free(tabd)
  rc = letkf_ctx_destroy(ctx)

  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) INT(nt, c_int32_t), INT(mn, c_int32_t)
  WRITE (u) mb, mr
  WRITE (u) anal_dev, anal_host
  WRITE (u) np_dev, np_host
  WRITE (u) obs%ensval(:, 1:nt), obs%val(1:nt), obs%ob_ri(1:nt), obs%ob_rj(1:nt), obs%ob_lev(1:nt), obs%ob_dat(1:nt), &
            obs%ob_err(1:nt)
  WRITE (u) qc, dat
  CLOSE (u)
END PROGRAM letkf_analysis_driver
