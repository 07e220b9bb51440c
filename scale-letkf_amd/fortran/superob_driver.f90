!===============================================================================
! superob_driver.f90 -- PROGRAM superob (scale/obs/superob.f90) end to end with the four stages on the device: the rows of all
! slots and their grid coordinates to the device, CALL superob_amd, download, and per slot the file supTT.dat of seven-value
! single-precision records (:992-998) with the unit conversions of :964-990.  Reads a case written by
! tests/test_fortran_superob.py.
!   file layout (little endian, stream):
!     int64 nobs ; int32 nlon, nlat, nlevx, nslots, nbslot, nobtype, nid, surface_typ_mask
!     int64 slot_off(0:nslots) ; int32 elem_uid(nid), method_g / _v / _t / _h (nobtype, nid)
!     int32 elm(nobs), typ(nobs) ; real64 lon, lat, lev, dat, err, ri, rj, rk (nobs each)
!   output: <prefix>TT.dat for TT = 01 .. nslots, sequential unformatted
!===============================================================================
PROGRAM superob_driver
  USE letkf_superob_amd
  IMPLICIT NONE
  INTEGER, PARAMETER :: id_u_obs = 2819, id_v_obs = 2820, id_t_obs = 3073, id_tv_obs = 3074, id_q_obs = 3330, id_rh_obs = 3331, &
                        id_ps_obs = 14593, id_tcmip_obs = 99993
  INTEGER(c_int64_t) :: nobs
  INTEGER(c_int64_t), TARGET :: nout(1)
  INTEGER(c_int32_t) :: h(8)
  INTEGER(c_int64_t), ALLOCATABLE, TARGET :: slot_off(:), slot_off_out(:)
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: elem_uid(:), mg(:, :), mv(:, :), mt(:, :), mh(:, :), elm(:), typ(:), oelm(:), otyp(:)
  REAL(c_double), ALLOCATABLE, TARGET :: v(:, :), ov(:, :)
  INTEGER :: u, uo, ios, ierr, islot, f
  INTEGER(c_int64_t) :: n
  INTEGER(c_size_t) :: nb4, nb8
  INTEGER(c_int) :: rc
  REAL(c_double) :: levout, datout, errout
  TYPE(c_ptr) :: ctx, d_in(10), d_out(14), d_nout, d_soff
  TYPE(letkf_superob_params) :: prm
  TYPE(letkf_superob_out) :: out
  CHARACTER(len=512) :: fin, prefix
  CHARACTER(len=2) :: tt

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, prefix)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) nobs
  READ (u) h
  ALLOCATE (slot_off(0:h(4)), slot_off_out(0:h(4)), elem_uid(h(7)), mg(h(6), h(7)), mv(h(6), h(7)), mt(h(6), h(7)), mh(h(6), h(7)))
  ALLOCATE (elm(nobs), typ(nobs), v(nobs, 8), oelm(nobs), otyp(nobs), ov(nobs, 5))
  READ (u) slot_off, elem_uid, mg, mv, mt, mh
  READ (u) elm, typ, v
  CLOSE (u)

  ! ---- the rows (what read_obs and phys2ijk leave) to the device, the outputs at capacity nobs
  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  nb4 = 4_c_size_t*nobs; nb8 = 8_c_size_t*nobs
  d_in(1) = up(c_loc(elm), nb4); d_in(2) = up(c_loc(typ), nb4)
  DO f = 1, 8
    d_in(2 + f) = up(c_loc(v(1, f)), nb8)
  END DO
  DO f = 1, 14
    CALL chk(hipMalloc(d_out(f), MAX(nb8, 8_c_size_t)), 'hipMalloc out')
  END DO
  CALL chk(hipMalloc(d_nout, 8_c_size_t), 'hipMalloc nout')
  CALL chk(hipMalloc(d_soff, 8_c_size_t*SIZE(slot_off)), 'hipMalloc slot_off_out')

  prm%nobs = nobs
  prm%elm = d_in(1); prm%typ = d_in(2); prm%lon = d_in(3); prm%lat = d_in(4); prm%lev = d_in(5); prm%dat = d_in(6)
  prm%err = d_in(7); prm%ri = d_in(8); prm%rj = d_in(9); prm%rk = d_in(10)
  prm%slot_off = c_loc(slot_off)
  prm%nlon = h(1); prm%nlat = h(2); prm%nlevx = h(3); prm%nslots = h(4); prm%nbslot = h(5); prm%nobtype = h(6); prm%nid = h(7)
  prm%surface_typ_mask = h(8)
  prm%elem_uid = c_loc(elem_uid)
  prm%method_g = c_loc(mg); prm%method_v = c_loc(mv); prm%method_t = c_loc(mt); prm%method_h = c_loc(mh)
  out%elm = d_out(1); out%typ = d_out(2); out%slot = d_out(3); out%lon = d_out(4); out%lat = d_out(5); out%lev = d_out(6)
  out%dat = d_out(7); out%err = d_out(8); out%ri = d_out(9); out%rj = d_out(10); out%rk = d_out(11)
  out%i = d_out(12); out%j = d_out(13); out%k = d_out(14)
  out%nout = d_nout; out%slot_off_out = d_soff
  out%qc1 = c_null_ptr; out%counts = c_null_ptr; out%obsnum = c_null_ptr

  CALL superob_amd(ctx, prm, out, ierr)
  CALL chk(INT(ierr, c_int), 'superob_amd')
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')               ! (the entry is asynchronous: before the download)
  CALL chk(hipMemcpy(c_loc(nout), d_nout, 8_c_size_t, hipMemcpyDeviceToHost), 'download nout')
  CALL chk(hipMemcpy(c_loc(slot_off_out), d_soff, 8_c_size_t*SIZE(slot_off), hipMemcpyDeviceToHost), 'download slot_off_out')
  IF (nout(1) > 0) THEN
    CALL chk(hipMemcpy(c_loc(oelm), d_out(1), 4_c_size_t*nout(1), hipMemcpyDeviceToHost), 'download elm')
    CALL chk(hipMemcpy(c_loc(otyp), d_out(2), 4_c_size_t*nout(1), hipMemcpyDeviceToHost), 'download typ')
    DO f = 1, 5
      CALL chk(hipMemcpy(c_loc(ov(1, f)), d_out(3 + f), 8_c_size_t*nout(1), hipMemcpyDeviceToHost), 'download rows')
    END DO
  END IF

  ! ---- :959-1003: the rows are already slot by slot
  DO islot = 1, h(4)
    WRITE (tt, '(I2.2)') islot
    OPEN (newunit=uo, file=trim(prefix)//tt//'.dat', form='unformatted', access='sequential', status='replace')
    DO n = slot_off_out(islot - 1) + 1, slot_off_out(islot)
      levout = ov(n, 3); datout = ov(n, 4); errout = ov(n, 5)
      SELECT CASE (oelm(n))
      CASE (id_u_obs, id_v_obs, id_t_obs, id_tv_obs, id_q_obs)
        levout = levout*0.01d0
      CASE (id_ps_obs, id_tcmip_obs)
        datout = datout*0.01d0
        errout = errout*0.01d0
      CASE (id_rh_obs)
        levout = levout*0.01d0
        datout = datout*100.0d0
        errout = errout*100.0d0
      END SELECT
      WRITE (uo) REAL(oelm(n), c_float), REAL(ov(n, 1), c_float), REAL(ov(n, 2), c_float), REAL(levout, c_float), &
                 REAL(datout, c_float), REAL(errout, c_float), REAL(otyp(n), c_float)
    END DO
    CLOSE (uo)
  END DO
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

END PROGRAM superob_driver
