!===============================================================================
! interp_window_driver.f90 -- das_letkf_interp_window_amd (letkf_interp_window_amd.f90) from a Fortran host.  Reads a case
! written by tests/test_fortran_interp_window.py (the arrays of one tile: its owned rectangle and the halo), uploads it,
! makes ONE call and writes the analysis array back; what the call does not own keeps the fill value -3.25.
!   file layout (little endian, stream):
!     int32 k, nv, nx, ny, nlev, stride_x, stride_y, nobs, kld, det_run ; int32 gnx, gny, gi0, gj0, oi0, oj0, onx, ony
!     real64 relax_alpha_spread
!     int32 nctype, ngroup, criterion, nlon, nlat, limit_hint ; real64 dx, dy, i_org, j_org, rain_base
!     the 20 arrays of letkf_search_tables in the struct's order, each as int64 nbytes + its bytes
!     real64 rig(nx*ny), rjg(nx*ny), rlev(npts), rz(npts), ensval(kld,nobs), dep(nobs), infl(npts*nv),
!            gues(npts,nens,nv)  perturbations in slots 1..k, the mean in k+1, the deterministic member in k+2
!===============================================================================
PROGRAM interp_window_driver
  USE letkf_interp_window_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: k, nv, nx, ny, nlev, sx, sy, nobs, kld, det_run, win(8)
  REAL(c_double) :: spread
  REAL(c_double), ALLOCATABLE, TARGET :: rig(:), rjg(:), rlev(:), rz(:), ensval(:, :), dep(:), infl(:), gues(:, :, :), &
                                         anal(:, :, :)
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: status(:)
  INTEGER(c_int8_t), ALLOCATABLE, TARGET :: raw(:)
  INTEGER :: u, ios, nens, i, ierr
  INTEGER(c_int64_t) :: npts, nbytes
  INTEGER(c_int) :: rc
  TYPE(c_ptr) :: ctx, d_rig, d_rjg, d_rlev, d_rz, d_ens, d_dep, d_infl, d_gues, d_anal, d_st, tp(20)
  TYPE(letkf_das_args) :: a
  TYPE(letkf_search_tables) :: t
  CHARACTER(len=512) :: fin, fout

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) k, nv, nx, ny, nlev, sx, sy, nobs, kld, det_run
  READ (u) win
  READ (u) spread
  READ (u) t%nctype, t%ngroup, t%criterion, t%nlon, t%nlat, t%limit_hint
  READ (u) t%dx, t%dy, t%i_org, t%j_org, t%rain_base
  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  DO i = 1, 20
    READ (u) nbytes
    ALLOCATE (raw(MAX(nbytes, 1_c_int64_t)))
    IF (nbytes > 0) READ (u) raw(1:nbytes)
    tp(i) = up(c_loc(raw), INT(MAX(nbytes, 1_c_int64_t), c_size_t))
    DEALLOCATE (raw)
  END DO
  t%group_start = tp(1); t%group_member = tp(2); t%vmode = tp(3); t%hori_loc = tp(4); t%vert_loc = tp(5)
  t%varloc = tp(6); t%max_nobs = tp(7); t%ngrd_i = tp(8); t%ngrd_j = tp(9); t%ngrdsch_i = tp(10); t%ngrdsch_j = tp(11)
  t%ngrdext_i = tp(12); t%ngrdext_j = tp(13); t%ac_off = tp(14); t%ac_ext = tp(15); t%ob_ri = tp(16); t%ob_rj = tp(17)
  t%ob_lev = tp(18); t%ob_dat = tp(19); t%ob_err = tp(20)
  npts = INT(nx, c_int64_t)*ny*nlev
  nens = k + 2
  ALLOCATE (rig(nx*ny), rjg(nx*ny), rlev(npts), rz(npts), ensval(kld, nobs), dep(nobs), infl(npts*nv), &
            gues(npts, nens, nv), anal(npts, nens, nv), status(npts))
  READ (u) rig, rjg, rlev, rz, ensval, dep, infl, gues
  CLOSE (u)

  d_rig = up(c_loc(rig), 8_c_size_t*nx*ny)
  d_rjg = up(c_loc(rjg), 8_c_size_t*nx*ny)
  d_rlev = up(c_loc(rlev), 8_c_size_t*npts)
  d_rz = up(c_loc(rz), 8_c_size_t*npts)
  d_ens = up(c_loc(ensval), 8_c_size_t*kld*nobs)
  d_dep = up(c_loc(dep), 8_c_size_t*nobs)
  d_infl = up(c_loc(infl), 8_c_size_t*npts*nv)
  d_gues = up(c_loc(gues), 8_c_size_t*npts*nens*nv)
  anal = -3.25d0
  d_anal = up(c_loc(anal), 8_c_size_t*npts*nens*nv)
  status = -1
  d_st = up(c_loc(status), 4_c_size_t*npts)

  a%k = k; a%nv = nv; a%det_run = det_run; a%infl_adaptive = 0; a%relax_to_inflated_prior = 0
  a%iv_p = 4; a%iv_q_first = 5; a%iv_q_last = MIN(10, nv - 1); a%warm_stride = 0
  a%relax_alpha = 0.0d0; a%relax_alpha_spread = spread; a%q_update_top = 0.0d0; a%q_sprd_max = 0.0d0
  a%npts = npts
  a%ensval = d_ens; a%kld = kld; a%dep = d_dep; a%beta = c_null_ptr; a%infl = d_infl; a%gues = d_gues; a%anal = d_anal
  a%sp = 1; a%sm = npts; a%sv = npts*nens
  a%status = d_st; a%rtps_infl_out = c_null_ptr
  a%warm_run = 0; a%var_mask = 0; a%infl_sv = 0
  CALL das_letkf_interp_window_amd(ctx, a, t, INT(nx), INT(ny), INT(nlev), INT(sx), INT(sy), d_rig, d_rjg, d_rlev, d_rz, &
                                   0_c_int64_t, c_null_ptr, INT(win(1)), INT(win(2)), INT(win(3)), INT(win(4)), &
                                   INT(win(5)), INT(win(6)), INT(win(7)), INT(win(8)), ierr)
  CALL chk(INT(ierr, c_int), 'das_letkf_interp_window_amd')
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
  CALL chk(hipMemcpy(c_loc(anal), d_anal, 8_c_size_t*npts*nens*nv, hipMemcpyDeviceToHost), 'download anal')
  CALL chk(hipMemcpy(c_loc(status), d_st, 4_c_size_t*npts, hipMemcpyDeviceToHost), 'download status')
  IF (COUNT(status == 0) /= INT(win(7))*INT(win(8))*nlev .OR. ANY(status > 0)) THEN   ! (-1: not owned, not written)
    WRITE (6, *) 'letkf_das_interp_window_dev: status 0 at', COUNT(status == 0), 'points, > 0 at', COUNT(status > 0)
    STOP 2
  END IF
  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) anal
  CLOSE (u)
  rc = letkf_ctx_destroy(ctx)

CONTAINS

  FUNCTION up(host, nbytes_) RESULT(d)
    TYPE(c_ptr), INTENT(IN) :: host
    INTEGER(c_size_t), INTENT(IN) :: nbytes_
    TYPE(c_ptr) :: d
    CALL chk(hipMalloc(d, nbytes_), 'hipMalloc')
    CALL chk(hipMemcpy(d, host, nbytes_, hipMemcpyHostToDevice), 'hipMemcpy H2D')
  END FUNCTION up

  SUBROUTINE chk(rc_, what)
    INTEGER(c_int), INTENT(IN) :: rc_
    CHARACTER(*), INTENT(IN) :: what
    IF (rc_ /= 0) THEN
      WRITE (6, *) 'error', rc_, 'in ', what
      STOP 5
    END IF
  END SUBROUTINE chk

END PROGRAM interp_window_driver
