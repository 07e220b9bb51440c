!===============================================================================
! mapproj_driver.f90 -- the rows of an observation file from lon / lat to obsda's lists, from a Fortran host:
!   CALL phys2ij per row (and MPRJ_rotcoef)  -> CALL phys2ij_amd: ri, rj and rotc per file row on the device
!   the first scan of obsope_cal             -> CALL obsscan_amd on those ri / rj, which never come back to the host
! Reads a case written by tests/test_fortran_mapproj.py, prints the tables bsn / bsna and writes ri, rj, rotc, bsn, bsna, set,
! idx and qc.
!   file layout (little endian, stream):
!     int32 nrow, nlon, nlat, ihalo, jhalo, prc_num_x, prc_num_y, slot_start, slot_end, slot_base     (nlon, nlat: of one subdomain)
!     real64 basepoint_lon, basepoint_lat, basepoint_x, basepoint_y, lc_lat1, lc_lat2, cxg1, cyg1, dx, dy, slot_tinterval
!     real64 lon(nrow), lat(nrow), dif(nrow)
!===============================================================================
PROGRAM mapproj_driver
  USE letkf_mapproj_amd
  USE letkf_obsscan_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: h(10)
  REAL(c_double) :: r(11)
  INTEGER(c_int64_t), TARGET :: off(2)
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: set(:), idx(:), qc(:), bsn(:, :), bsna(:, :)
  REAL(c_double), ALLOCATABLE, TARGET :: lon(:), lat(:), dif(:), ri(:), rj(:), rotc(:, :)
  INTEGER :: u, ios, nrow, nprocs, s0, s1, ip, ierr
  INTEGER(c_int) :: rc
  TYPE(c_ptr) :: ctx, d_lon, d_lat, d_dif, d_ri, d_rj, d_rotc, d_set, d_idx, d_qc
  TYPE(letkf_mapproj) :: proj
  TYPE(letkf_obsscan_params) :: sp
  CHARACTER(len=512) :: fin, fout

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) h
  READ (u) r
  nrow = h(1); nprocs = h(6)*h(7); s0 = h(8); s1 = h(9)
  ALLOCATE (lon(nrow), lat(nrow), dif(nrow), ri(nrow), rj(nrow), rotc(2, nrow), set(nrow), idx(nrow), qc(nrow), &
            bsn(s0:s1 + 2, 0:nprocs - 1), bsna(s0 - 1:s1 + 2, 0:nprocs - 1))
  READ (u) lon, lat, dif
  CLOSE (u)

  ! ---- MPRJ_setup's values, once, on the host
  CALL mapproj_setup_amd(r(1), r(2), r(3), r(4), r(5), r(6), r(7), r(8), r(9), r(10), proj, ierr)
  CALL chk(INT(ierr, c_int), 'mapproj_setup_amd')

  ! ---- the file's rows go up as the file holds them; ri / rj / rotc are made where the scan and the operator read them
  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  d_lon = up(c_loc(lon), 8_c_size_t*nrow); d_lat = up(c_loc(lat), 8_c_size_t*nrow); d_dif = up(c_loc(dif), 8_c_size_t*nrow)
  ri = 0.0d0; rj = 0.0d0; rotc = 0.0d0; set = 0; idx = 0; qc = 0
  d_ri = up(c_loc(ri), 8_c_size_t*nrow); d_rj = up(c_loc(rj), 8_c_size_t*nrow); d_rotc = up(c_loc(rotc), 16_c_size_t*nrow)
  d_set = up(c_loc(set), 4_c_size_t*nrow); d_idx = up(c_loc(idx), 4_c_size_t*nrow); d_qc = up(c_loc(qc), 4_c_size_t*nrow)
  CALL phys2ij_amd(ctx, proj, INT(nrow, c_int64_t), d_lon, d_lat, d_ri, d_rj, ierr, rotc=d_rotc)
  CALL chk(INT(ierr, c_int), 'phys2ij_amd')

  ! ---- the first scan, on the same stream
  off(1) = 0; off(2) = nrow
  sp%obsda_run = c_null_ptr
  sp%nlon = h(2); sp%nlat = h(3); sp%ihalo = h(4); sp%jhalo = h(5); sp%prc_num_x = h(6); sp%prc_num_y = h(7)
  sp%slot_start = s0; sp%slot_end = s1; sp%slot_base = h(10); sp%myrank_d = 0; sp%slot_tinterval = r(11)
  CALL obsscan_amd(ctx, sp, 1, off, d_ri, d_rj, d_dif, d_set, d_idx, d_qc, bsn, bsna, ierr)
  CALL chk(INT(ierr, c_int), 'obsscan_amd')
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')

  DO ip = 0, nprocs - 1
    WRITE (6, '(A,I4,A,20I7)') 'subdomain', ip, ' bsn ', bsn(:, ip)
    WRITE (6, '(A,I4,A,20I7)') 'subdomain', ip, ' bsna', bsna(:, ip)
  END DO
  CALL chk(hipMemcpy(c_loc(ri), d_ri, 8_c_size_t*nrow, hipMemcpyDeviceToHost), 'download ri')
  CALL chk(hipMemcpy(c_loc(rj), d_rj, 8_c_size_t*nrow, hipMemcpyDeviceToHost), 'download rj')
  CALL chk(hipMemcpy(c_loc(rotc), d_rotc, 16_c_size_t*nrow, hipMemcpyDeviceToHost), 'download rotc')
  CALL chk(hipMemcpy(c_loc(set), d_set, 4_c_size_t*nrow, hipMemcpyDeviceToHost), 'download set')
  CALL chk(hipMemcpy(c_loc(idx), d_idx, 4_c_size_t*nrow, hipMemcpyDeviceToHost), 'download idx')
  CALL chk(hipMemcpy(c_loc(qc), d_qc, 4_c_size_t*nrow, hipMemcpyDeviceToHost), 'download qc')
  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) ri, rj, rotc, bsn, bsna, set, idx, qc
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

END PROGRAM mapproj_driver
