!===============================================================================
! efso_locadv_driver.f90 -- a Fortran host calling das_efso_amd (letkf_tools_amd.f90) with localisation advection for
! two variable-localisation classes that accumulate into one djdy: reads the search tables, the points, the EFSO inputs
! and the winds from a case file written by tests/test_fortran_efso_locadv.py, uploads the tables (what
! set_letkf_obs_amd would leave on the device), makes the two calls and writes djdy and obsense.  hdr(17) = 1 passes the
! advection arguments (u0, v0, u1, v1, locadv_rate, eft, dx, dy), 0 leaves them out.
!   file (little endian, stream): int32 hdr(17); real64 r(7); then the arrays in the order read below
!===============================================================================
PROGRAM efso_locadv_driver
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_tools_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: hdr(17)
  REAL(c_double) :: r(7)
  INTEGER :: nctype, ngroup, nij1, nlev, member, nv3d, nterm, nobs, kld, nacx, mask1, mask2, ngm, u, ios
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: gs(:), gm(:), vmode(:), mx(:), gi(:), gj(:), si(:), sj(:), ei(:), ej(:), ace(:)
  INTEGER(c_int32_t), ALLOCATABLE :: term32(:)
  INTEGER, ALLOCATABLE :: term_of_var(:)
  INTEGER(c_int64_t), ALLOCATABLE, TARGET :: aco(:)
  REAL(c_double), ALLOCATABLE, TARGET :: hl(:), vl(:), vloc(:), ori(:), orj(:), olev(:), odat(:), oerr(:)
  REAL(c_double), ALLOCATABLE :: rig1(:), rjg1(:), rlev(:, :), hgt1(:, :), fcst3d(:, :, :, :), fcer3d(:, :, :), ya(:, :), &
                                 dep(:), djdy(:, :), obsense(:, :), u0(:, :), v0(:, :), u1(:, :), v1(:, :)
  TYPE(letkf_search_tables) :: t
  TYPE(c_ptr) :: ctx
  CHARACTER(len=512) :: fin, fout
  INTEGER(c_int) :: rc

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) hdr
  READ (u) r
  nctype = hdr(1); ngroup = hdr(2); nij1 = hdr(6); nlev = hdr(7); member = hdr(8); nv3d = hdr(9); nterm = hdr(10)
  nobs = hdr(11); kld = hdr(12); nacx = hdr(13); mask1 = hdr(14); mask2 = hdr(15); ngm = hdr(16)
  ALLOCATE (gs(ngroup + 1), gm(ngm), vmode(nctype), mx(nctype), gi(nctype), gj(nctype), si(nctype), sj(nctype), ei(nctype), &
            ej(nctype), term32(nv3d), term_of_var(nv3d), aco(nctype), ace(nacx), hl(nctype), vl(nctype), vloc(nctype), &
            ori(nobs), orj(nobs), olev(nobs), odat(nobs), oerr(nobs), rig1(nij1), rjg1(nij1), rlev(nij1, nlev), hgt1(nij1, nlev), &
            fcst3d(nij1, nlev, member, nv3d), fcer3d(nij1, nlev, nv3d), ya(kld, nobs), dep(nobs), djdy(nterm, nobs), &
            obsense(nterm, nobs), u0(nij1, nlev), v0(nij1, nlev), u1(nij1, nlev), v1(nij1, nlev))
  READ (u) gs, gm, vmode, mx, gi, gj, si, sj, ei, ej, term32
  READ (u) aco
  READ (u) ace
  READ (u) hl, vl, vloc, ori, orj, olev, odat, oerr, rig1, rjg1, rlev, hgt1, fcst3d, fcer3d, ya, dep, u0, v0, u1, v1
  CLOSE (u)
  term_of_var = term32

  t%nctype = nctype; t%ngroup = ngroup; t%criterion = hdr(3); t%nlon = hdr(4); t%nlat = hdr(5)
  t%limit_hint = MERGE(2, 1, ANY(mx > 0))
  t%dx = r(1); t%dy = r(2); t%i_org = r(3); t%j_org = r(4); t%rain_base = r(5)
  t%group_start = up(c_loc(gs), 4_c_size_t*SIZE(gs)); t%group_member = up(c_loc(gm), 4_c_size_t*SIZE(gm))
  t%vmode = up(c_loc(vmode), 4_c_size_t*nctype); t%max_nobs = up(c_loc(mx), 4_c_size_t*nctype)
  t%hori_loc = up(c_loc(hl), 8_c_size_t*nctype); t%vert_loc = up(c_loc(vl), 8_c_size_t*nctype)
  t%varloc = up(c_loc(vloc), 8_c_size_t*nctype)
  t%ngrd_i = up(c_loc(gi), 4_c_size_t*nctype); t%ngrd_j = up(c_loc(gj), 4_c_size_t*nctype)
  t%ngrdsch_i = up(c_loc(si), 4_c_size_t*nctype); t%ngrdsch_j = up(c_loc(sj), 4_c_size_t*nctype)
  t%ngrdext_i = up(c_loc(ei), 4_c_size_t*nctype); t%ngrdext_j = up(c_loc(ej), 4_c_size_t*nctype)
  t%ac_off = up(c_loc(aco), 8_c_size_t*nctype); t%ac_ext = up(c_loc(ace), 4_c_size_t*nacx)
  t%ob_ri = up(c_loc(ori), 8_c_size_t*nobs); t%ob_rj = up(c_loc(orj), 8_c_size_t*nobs)
  t%ob_lev = up(c_loc(olev), 8_c_size_t*nobs); t%ob_dat = up(c_loc(odat), 8_c_size_t*nobs)
  t%ob_err = up(c_loc(oerr), 8_c_size_t*nobs)

  rc = letkf_ctx_create(0_c_int, ctx)
  IF (rc /= 0) STOP 4
  djdy = 0.0d0
  IF (hdr(17) == 1) THEN
    CALL das_efso_amd(ctx, t, nij1, nlev, member, nv3d, rig1, rjg1, rlev, hgt1, fcst3d, fcer3d, nterm, term_of_var, kld, nobs, &
                      ya, dep, djdy, obsense, var_mask=mask1, u0=u0, v0=v0, u1=u1, v1=v1, locadv_rate=r(6), eft=r(7), &
                      dx=r(1), dy=r(2))
    CALL das_efso_amd(ctx, t, nij1, nlev, member, nv3d, rig1, rjg1, rlev, hgt1, fcst3d, fcer3d, nterm, term_of_var, kld, nobs, &
                      ya, dep, djdy, obsense, var_mask=mask2, u0=u0, v0=v0, u1=u1, v1=v1, locadv_rate=r(6), eft=r(7), &
                      dx=r(1), dy=r(2))
  ELSE
    CALL das_efso_amd(ctx, t, nij1, nlev, member, nv3d, rig1, rjg1, rlev, hgt1, fcst3d, fcer3d, nterm, term_of_var, kld, nobs, &
                      ya, dep, djdy, obsense, var_mask=mask1)
    CALL das_efso_amd(ctx, t, nij1, nlev, member, nv3d, rig1, rjg1, rlev, hgt1, fcst3d, fcer3d, nterm, term_of_var, kld, nobs, &
                      ya, dep, djdy, obsense, var_mask=mask2)
  END IF
  rc = letkf_ctx_destroy(ctx)

  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) djdy
  WRITE (u) obsense
  CLOSE (u)

CONTAINS

  FUNCTION up(host, nbytes) RESULT(d)
    TYPE(c_ptr), INTENT(IN) :: host
    INTEGER(c_size_t), INTENT(IN) :: nbytes
    TYPE(c_ptr) :: d
    IF (hipMalloc(d, MAX(nbytes, 8_c_size_t)) /= 0) STOP 5
    IF (hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice) /= 0) STOP 5
  END FUNCTION up

END PROGRAM efso_locadv_driver
