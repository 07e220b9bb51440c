!===============================================================================
! nobsout_driver.f90 -- das_letkf's main loop with NOBS_OUT called from Fortran (INTEGRATION.md level 2): one
! letkf_das_columns_nobs_dev call for a subdomain, then nobs_fields_amd for work3dn and the eleven fields.  Reads a case written by
! tests/test_fortran_nobsout.py, uploads it, runs the two entries, downloads and writes the results.
!   file layout (little endian, stream):
!     int32 k, nv, nij1, nlev, nobs, kld, nctype, ngroup, criterion, nlon, nlat, nobtype ; int64 list_bytes, nac
!     real64 dx, dy, i_org, j_org, rain_base, relax_alpha_spread
!     int32 group_start(ngroup+1), group_member(nctype), vmode, max_nobs, ngrd_i, ngrd_j, ngrdsch_i, ngrdsch_j, ngrdext_i,
!           ngrdext_j, elm_u_ctype, typ_ctype (nctype each)
!     real64 hori_loc, vert_loc, varloc (nctype each) ; int64 ac_off(nctype) ; int32 ac_ext(nac)
!     real64 ob_ri, ob_rj, ob_lev, ob_dat, ob_err (nobs each)
!     real64 rig(nij1), rjg(nij1), rlev(nij1*nlev), rz(nij1*nlev)
!     real64 ensval(kld,nobs), dep(nobs), beta(nij1*nlev), infl(nij1*nlev*nv)
!     real64 gues(nij1*nlev, k+1, nv): the perturbations in slots 1..k, the mean in slot k+1
!   output: int32 nobs_out(npts), nobs_ctype(nctype,npts) ; real64 cutd_ctype(nctype,npts), work3dn(nobtype+6,npts),
!           work3d(npts,11), anal(npts,k+1,nv)
!===============================================================================
PROGRAM nobsout_driver
  USE letkf_nobsout_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: k, nv, nij1, nlev, nobs, kld, nctype, ngroup, criterion, nlon, nlat, nobtype
  INTEGER(c_int64_t) :: list_bytes, nac, npts
  REAL(c_double) :: dx, dy, i_org, j_org, rain_base, alpha
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: group_start(:), group_member(:), ic4(:, :), elm_u(:), typ(:), ac_ext(:), status(:), &
                                             nobs_out(:), nobs_ct(:, :)
  INTEGER(c_int64_t), ALLOCATABLE, TARGET :: ac_off(:)
  REAL(c_double), ALLOCATABLE, TARGET :: loc3(:, :), ob(:, :), rig(:), rjg(:), rlev(:), rz(:), ensval(:, :), dep(:), beta(:), &
                                         infl(:), gues(:, :, :), anal(:, :, :), cutd_ct(:, :), work3dn(:, :), work3d(:, :)
  INTEGER :: u, ios, nens, ierr, q
  INTEGER(c_int) :: rc
  TYPE(c_ptr) :: ctx, d_ic4(8), d_loc3(3), d_ob(5), d_rig, d_rjg, d_rlev, d_rz, d_ens, d_dep, d_beta, d_infl, d_gues, d_anal, &
                 d_st, d_nobs, d_nct, d_cut, d_w3n, d_w3
  TYPE(letkf_das_args) :: a
  TYPE(letkf_search_tables) :: t
  CHARACTER(len=512) :: fin, fout

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) k, nv, nij1, nlev, nobs, kld, nctype, ngroup, criterion, nlon, nlat, nobtype
  READ (u) list_bytes, nac
  READ (u) dx, dy, i_org, j_org, rain_base, alpha
  npts = INT(nij1, c_int64_t)*nlev
  nens = k + 1
  ! ic4: vmode, max_nobs, ngrd_i, ngrd_j, ngrdsch_i, ngrdsch_j, ngrdext_i, ngrdext_j; loc3: hori_loc, vert_loc, varloc
  ALLOCATE (group_start(ngroup + 1), group_member(nctype), ic4(nctype, 8), elm_u(nctype), typ(nctype), loc3(nctype, 3), &
            ac_off(nctype), ac_ext(nac), ob(nobs, 5), rig(nij1), rjg(nij1), rlev(npts), rz(npts), ensval(kld, nobs), dep(nobs), &
            beta(npts), infl(npts*nv), gues(npts, nens, nv), anal(npts, nens, nv), status(npts), nobs_out(npts), &
            nobs_ct(nctype, npts), cutd_ct(nctype, npts), work3dn(nobtype + 6, npts), work3d(npts, LETKF_NOBSOUT_NFIELDS))
  READ (u) group_start, group_member, ic4, elm_u, typ
  READ (u) loc3, ac_off, ac_ext
  READ (u) ob, rig, rjg, rlev, rz
  READ (u) ensval, dep, beta, infl, gues
  CLOSE (u)

  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  t%nctype = nctype; t%ngroup = ngroup; t%criterion = criterion; t%nlon = nlon; t%nlat = nlat; t%limit_hint = 0
  t%dx = dx; t%dy = dy; t%i_org = i_org; t%j_org = j_org; t%rain_base = rain_base
  t%group_start = up(c_loc(group_start), 4_c_size_t*(ngroup + 1))
  t%group_member = up(c_loc(group_member), 4_c_size_t*nctype)
  DO q = 1, 8
    d_ic4(q) = up(c_loc(ic4(1, q)), 4_c_size_t*nctype)
  END DO
  DO q = 1, 3
    d_loc3(q) = up(c_loc(loc3(1, q)), 8_c_size_t*nctype)
  END DO
  DO q = 1, 5
    d_ob(q) = up(c_loc(ob(1, q)), 8_c_size_t*MAX(nobs, 1))
  END DO
  t%vmode = d_ic4(1); t%max_nobs = d_ic4(2); t%ngrd_i = d_ic4(3); t%ngrd_j = d_ic4(4); t%ngrdsch_i = d_ic4(5)
  t%ngrdsch_j = d_ic4(6); t%ngrdext_i = d_ic4(7); t%ngrdext_j = d_ic4(8)
  t%hori_loc = d_loc3(1); t%vert_loc = d_loc3(2); t%varloc = d_loc3(3)
  t%ac_off = up(c_loc(ac_off), 8_c_size_t*nctype)
  t%ac_ext = up(c_loc(ac_ext), 4_c_size_t*nac)
  t%ob_ri = d_ob(1); t%ob_rj = d_ob(2); t%ob_lev = d_ob(3); t%ob_dat = d_ob(4); t%ob_err = d_ob(5)
  d_rig = up(c_loc(rig), 8_c_size_t*nij1)
  d_rjg = up(c_loc(rjg), 8_c_size_t*nij1)
  d_rlev = up(c_loc(rlev), 8_c_size_t*npts)
  d_rz = up(c_loc(rz), 8_c_size_t*npts)
  d_ens = up(c_loc(ensval), 8_c_size_t*kld*MAX(nobs, 1))
  d_dep = up(c_loc(dep), 8_c_size_t*MAX(nobs, 1))
  d_beta = up(c_loc(beta), 8_c_size_t*npts)
  d_infl = up(c_loc(infl), 8_c_size_t*npts*nv)
  d_gues = up(c_loc(gues), 8_c_size_t*npts*nens*nv)
  anal = 0.0d0; status = -1; nobs_out = -1; nobs_ct = -1; cutd_ct = -1.0d0; work3dn = -1.0d0; work3d = -1.0d0
  d_anal = up(c_loc(anal), 8_c_size_t*npts*nens*nv)
  d_st = up(c_loc(status), 4_c_size_t*npts)
  d_nobs = up(c_loc(nobs_out), 4_c_size_t*npts)
  d_nct = up(c_loc(nobs_ct), 4_c_size_t*npts*nctype)
  d_cut = up(c_loc(cutd_ct), 8_c_size_t*npts*nctype)
  d_w3n = up(c_loc(work3dn), 8_c_size_t*npts*(nobtype + 6))
  d_w3 = up(c_loc(work3d), 8_c_size_t*npts*LETKF_NOBSOUT_NFIELDS)

  a%k = k; a%nv = nv; a%det_run = 0; a%infl_adaptive = 0; a%relax_to_inflated_prior = 0
  a%iv_p = 4; a%iv_q_first = 5; a%iv_q_last = MIN(10, nv - 1); a%warm_stride = 0
  a%relax_alpha = 0.0d0; a%relax_alpha_spread = alpha; a%q_update_top = 0.0d0; a%q_sprd_max = 0.0d0
  a%npts = npts
  a%obs_off = c_null_ptr; a%obs_idx = c_null_ptr; a%rdiag_l = c_null_ptr; a%rloc_l = c_null_ptr
  a%ensval = d_ens; a%kld = kld; a%dep = d_dep; a%beta = d_beta; a%infl = d_infl; a%gues = d_gues; a%anal = d_anal
  a%sp = 1; a%sm = npts; a%sv = npts*nens
  a%trans_out = c_null_ptr; a%transm_out = c_null_ptr; a%pa_out = c_null_ptr
  a%status = d_st; a%nsweep = c_null_ptr; a%rtps_infl_out = c_null_ptr
  a%warm_run = 0; a%var_mask = 0; a%infl_sv = 0
  ! the three lines that stand where CALL letkf_das_columns_dev stood
  CALL chk(letkf_das_columns_nobs_dev(ctx, a, t, INT(nij1, c_int64_t), nlev, d_rig, d_rjg, d_rlev, d_rz, list_bytes, d_nobs, &
                                      d_nct, d_cut), 'das_columns_nobs')
  CALL nobs_fields_amd(ctx, INT(nctype), elm_u, typ, INT(nobtype), npts, d_nct, d_cut, d_w3n, d_w3, ierr)
  CALL chk(INT(ierr, c_int), 'nobs_fields')
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')

  CALL chk(hipMemcpy(c_loc(status), d_st, 4_c_size_t*npts, hipMemcpyDeviceToHost), 'download status')
  CALL chk(hipMemcpy(c_loc(nobs_out), d_nobs, 4_c_size_t*npts, hipMemcpyDeviceToHost), 'download nobs_out')
  CALL chk(hipMemcpy(c_loc(nobs_ct), d_nct, 4_c_size_t*npts*nctype, hipMemcpyDeviceToHost), 'download nobs_ctype')
  CALL chk(hipMemcpy(c_loc(cutd_ct), d_cut, 8_c_size_t*npts*nctype, hipMemcpyDeviceToHost), 'download cutd_ctype')
  CALL chk(hipMemcpy(c_loc(work3dn), d_w3n, 8_c_size_t*npts*(nobtype + 6), hipMemcpyDeviceToHost), 'download work3dn')
  CALL chk(hipMemcpy(c_loc(work3d), d_w3, 8_c_size_t*npts*LETKF_NOBSOUT_NFIELDS, hipMemcpyDeviceToHost), 'download work3d')
  CALL chk(hipMemcpy(c_loc(anal), d_anal, 8_c_size_t*npts*nens*nv, hipMemcpyDeviceToHost), 'download anal')
  IF (ANY(status /= 0)) THEN
    WRITE (6, *) 'letkf_das_columns_nobs_dev: non-zero status at', COUNT(status /= 0), 'points'
    STOP 2
  END IF
  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) nobs_out, nobs_ct, cutd_ct, work3dn, work3d, anal
  CLOSE (u)
  rc = letkf_ctx_destroy(ctx)

CONTAINS

  FUNCTION up(host, nbytes) RESULT(d)
    TYPE(c_ptr), INTENT(IN) :: host
    INTEGER(c_size_t), INTENT(IN) :: nbytes
    TYPE(c_ptr) :: d
    CALL chk(hipMalloc(d, MAX(nbytes, 8_c_size_t)), 'hipMalloc')
    IF (nbytes > 0) CALL chk(hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice), 'hipMemcpy H2D')
  END FUNCTION up

  SUBROUTINE chk(rc_, what)
    INTEGER(c_int), INTENT(IN) :: rc_
    CHARACTER(*), INTENT(IN) :: what
    IF (rc_ /= 0) THEN
      WRITE (6, *) 'error', rc_, 'in ', what
      STOP 5
    END IF
  END SUBROUTINE chk

END PROGRAM nobsout_driver
