!===============================================================================
! obssim_driver.f90 -- the `restart` branch of PROGRAM obssim (scale/obs/obssim.f90:79-100) end to end on one subdomain, with the
! state on the device:  CALL state_to_history_amd (what read_restart + state_to_history do), CALL obssim_cal_amd with stggrd = 1
! and the records as the output, download, and write_grd_mpi's direct-access GrADS file record by record (one subdomain: the
! MPI_REDUCE is the identity).  Reads a case written by tests/test_fortran_obssim.py.
!   file layout (little endian, stream):
!     int32 nlev, nlon, nlat, khalo, ihalo, jhalo, nv3d, edge_fill, method, use_tv, nvar3, nvar2, has_rotc, 0, 0, 0
!     int32 vars3(16), vars2(16)
!     real64 radar_lon, radar_lat, radar_z, min_radar_ref_dbz, low_ref_shift, ps_adjust_thres, ztop, 0
!     real64 cz(nlev), topo(nlon,nlat), x(nlon,nlat,nlev,nv3d), lon(nlon,nlat), lat(nlon,nlat), rotc(2,nlon,nlat)
!   output: the GrADS file, nvar3 * nlev + nvar2 records of real32 (nlon, nlat)
!===============================================================================
PROGRAM obssim_driver
  USE letkf_monit_amd
  USE letkf_obssim_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: h(16), vars3(16), vars2(16)
  REAL(c_double) :: r(8)
  REAL(c_double), ALLOCATABLE, TARGET :: cz(:), topo(:, :), x(:, :, :, :), lon(:, :), lat(:, :), rotc(:, :, :)
  REAL(c_float), ALLOCATABLE, TARGET :: bufr4(:, :, :)
  INTEGER :: u, uo, ios, nlev, nlon, nlat, khalo, ihalo, jhalo, nv3d, nlevh, nlonh, nlath, nrec, irec, iolen, ierr
  INTEGER(c_int) :: rc
  TYPE(c_ptr) :: ctx, d_topo, d_x, d_lon, d_lat, d_rotc, d_v3, d_v2, d_rec
  TYPE(letkf_obsope_fields) :: fl
  TYPE(letkf_hist_state) :: st
  TYPE(letkf_obssim_params) :: prm
  CHARACTER(len=512) :: fin, fout

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) h
  READ (u) vars3, vars2
  READ (u) r
  nlev = h(1); nlon = h(2); nlat = h(3); khalo = h(4); ihalo = h(5); jhalo = h(6); nv3d = h(7)
  nlevh = nlev + 2*khalo; nlonh = nlon + 2*ihalo; nlath = nlat + 2*jhalo
  nrec = h(11)*nlev + h(12)
  ALLOCATE (cz(nlev), topo(nlon, nlat), x(nlon, nlat, nlev, nv3d), lon(nlon, nlat), lat(nlon, nlat), rotc(2, nlon, nlat), &
            bufr4(nlon, nlat, nrec))
  READ (u) cz, topo, x, lon, lat, rotc
  CLOSE (u)

  ! ---- the state (what read_restart leaves), the projection's lon / lat / rotc: to the device once
  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  d_topo = up(c_loc(topo), 8_c_size_t*SIZE(topo)); d_x = up(c_loc(x), 8_c_size_t*SIZE(x))
  d_lon = up(c_loc(lon), 8_c_size_t*SIZE(lon)); d_lat = up(c_loc(lat), 8_c_size_t*SIZE(lat))
  d_rotc = up(c_loc(rotc), 8_c_size_t*SIZE(rotc))
  CALL chk(hipMalloc(d_v3, 8_c_size_t*nlevh*nlonh*nlath*13), 'hipMalloc v3d')
  CALL chk(hipMalloc(d_v2, 8_c_size_t*nlonh*nlath*7), 'hipMalloc v2d')
  CALL chk(hipMalloc(d_rec, 4_c_size_t*SIZE(bufr4)), 'hipMalloc rec')

  fl%nlev = nlev; fl%nlon = nlon; fl%nlat = nlat; fl%khalo = khalo; fl%ihalo = ihalo; fl%jhalo = jhalo
  fl%nv3dd = 13; fl%nv2dd = 7; fl%nmem = 1; fl%m0 = 0
  fl%v3d = d_v3; fl%s3k = 1; fl%s3i = nlevh; fl%s3j = INT(nlevh, c_int64_t)*nlonh; fl%s3v = fl%s3j*nlath; fl%s3m = fl%s3v*13
  fl%v2d = d_v2; fl%s2i = 1; fl%s2j = nlonh; fl%s2v = INT(nlonh, c_int64_t)*nlath; fl%s2m = fl%s2v*7
  st%nv3d = nv3d; st%edge_fill = h(8); st%x = d_x
  st%si = 1; st%sj = nlon; st%sl = INT(nlon, c_int64_t)*nlat; st%sv = st%sl*nlev
  st%topo = d_topo; st%cz = c_loc(cz); st%ztop = r(7)
  prm%nvar3 = h(11); prm%vars3 = vars3; prm%nvar2 = h(12); prm%vars2 = vars2
  prm%radar_lon = r(1); prm%radar_lat = r(2); prm%radar_z = r(3)
  prm%lon = d_lon; prm%lat = d_lat; prm%rotc = c_null_ptr
  IF (h(13) /= 0) prm%rotc = d_rotc
  prm%method_ref_calc = h(9); prm%use_terminal_velocity = h(10); prm%stggrd = 1; prm%round_single = 1
  prm%min_radar_ref_dbz = r(4); prm%low_ref_shift = r(5); prm%ps_adjust_thres = r(6)

  ! ---- call state_to_history(v3dg, v2dg, topo, v3dgh, v2dgh) ; call obssim_cal(v3dgh, v2dgh, v3dgsim, v2dgsim, stggrd=1)
  CALL state_to_history_amd(ctx, st, fl, d_v3, d_v2, ierr)
  CALL chk(INT(ierr, c_int), 'state_to_history_amd')
  CALL obssim_cal_amd(ctx, fl, c_null_ptr, c_null_ptr, 1, prm, d_rec, ierr)
  CALL chk(INT(ierr, c_int), 'obssim_cal_amd')
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')               ! (the entry is asynchronous: before the download)
  CALL chk(hipMemcpy(c_loc(bufr4), d_rec, 4_c_size_t*SIZE(bufr4), hipMemcpyDeviceToHost), 'download rec')

  ! ---- write_grd_mpi(filename, nv3dgrd, nv2dgrd, step = 1, ...): the records are already in its order
  INQUIRE (iolength=iolen) bufr4(:, :, 1)
  OPEN (newunit=uo, file=trim(fout), form='unformatted', access='direct', status='replace', recl=iolen)
  DO irec = 1, nrec
    WRITE (uo, rec=irec) bufr4(:, :, irec)
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

END PROGRAM obssim_driver
