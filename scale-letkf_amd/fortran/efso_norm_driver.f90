!===============================================================================
! efso_norm_driver.f90 -- EFSO from the forecast fields to the impact table, from a Fortran host: efso_norm_amd (the fcer
! assembly and lnorm), das_efso_amd (djdy and obsense), print_obsense_amd (the table on standard output).  Reads the
! search tables, the points, the forecast fields, the observations and the names from a case file written by
! tests/test_fortran_efso_norm.py, uploads the tables (what set_letkf_obs_amd would leave on the device) and writes the
! normed fields, obsense and the tables of every term.
!   file (little endian, stream): int32 hdr(18); real64 r(11); then the arrays in the order read below
!===============================================================================
PROGRAM efso_norm_driver
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_tools_amd
  USE efso_tools_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: hdr(18)
  REAL(c_double) :: r(11)
  INTEGER :: nctype, ngroup, nij1, nlev, member, nv3d, nterm, nobs, nacx, ngm, nid, nobtype, u, ios
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: gs(:), gm(:), vmode(:), mx(:), gi(:), gj(:), si(:), sj(:), ei(:), ej(:), ace(:)
  INTEGER(c_int32_t), ALLOCATABLE :: term32(:), elm(:), typ(:), uid(:), cnt(:, :, :), neg(:, :, :, :)
  INTEGER, ALLOCATABLE :: term_of_var(:)
  INTEGER(c_int64_t), ALLOCATABLE, TARGET :: aco(:)
  REAL(c_double), ALLOCATABLE, TARGET :: hl(:), vl(:), vloc(:), ori(:), orj(:), olev(:), odat(:), oerr(:)
  REAL(c_double), ALLOCATABLE :: rig1(:), rjg1(:), rlev(:, :), hgt1(:, :), fcst3d(:, :, :, :), fcer3d(:, :, :), xf(:, :, :), &
                                 xg(:, :, :), xa(:, :, :), wg1(:), lon1(:), lat1(:), ya(:, :), dep(:), olat(:), djdy(:, :), &
                                 obsense(:, :), ssum(:, :, :, :)
  CHARACTER(len=6), ALLOCATABLE :: otl(:)
  CHARACTER(len=3), ALLOCATABLE :: oel(:)
  TYPE(letkf_search_tables) :: t
  TYPE(efso_norm_nml) :: nml
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
  nobs = hdr(11); nacx = hdr(12); ngm = hdr(13); nid = hdr(14); nobtype = hdr(15)
  ALLOCATE (gs(ngroup + 1), gm(ngm), vmode(nctype), mx(nctype), gi(nctype), gj(nctype), si(nctype), sj(nctype), ei(nctype), &
            ej(nctype), term32(nv3d), term_of_var(nv3d), aco(nctype), ace(nacx), hl(nctype), vl(nctype), vloc(nctype), &
            ori(nobs), orj(nobs), olev(nobs), odat(nobs), oerr(nobs), rig1(nij1), rjg1(nij1), rlev(nij1, nlev), hgt1(nij1, nlev), &
            fcst3d(nij1, nlev, member, nv3d), fcer3d(nij1, nlev, nv3d), xf(nij1, nlev, nv3d), xg(nij1, nlev, nv3d), &
            xa(nij1, nlev, nv3d), wg1(nij1), lon1(nij1), lat1(nij1), ya(member, nobs), dep(nobs), olat(nobs), elm(nobs), &
            typ(nobs), uid(nid), otl(nobtype), oel(nid), djdy(nterm, nobs), obsense(nterm, nobs), &
            cnt(nid, nobtype + 1, 3), ssum(nid, nobtype + 1, 3, nterm), neg(nid, nobtype + 1, 3, nterm))
  READ (u) gs, gm, vmode, mx, gi, gj, si, sj, ei, ej, term32
  READ (u) aco
  READ (u) ace
  READ (u) hl, vl, vloc, ori, orj, olev, odat, oerr, rig1, rjg1, rlev, hgt1, fcst3d, xf, xg, xa, wg1, lon1, lat1, ya, dep, olat
  READ (u) elm, typ, uid
  READ (u) otl, oel
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

  nml%tar_minlev = hdr(16); nml%tar_maxlev = hdr(17)
  nml%wmoist = r(6); nml%tar_minlon = r(7); nml%tar_maxlon = r(8); nml%tar_minlat = r(9); nml%tar_maxlat = r(10)

  rc = letkf_ctx_create(0_c_int, ctx)
  IF (rc /= 0) STOP 4
  ! efso.f90:100-120: the forecast error from the three means, then the norm
  fcer3d = 0.0d0
  IF (hdr(18) == 1) THEN
    CALL efso_norm_amd(ctx, nml, nij1, nlev, member, nv3d, fcst3d, fcer3d, xf3d=xf, xg3d=xg, xa3d=xa, wg1=wg1, lon1=lon1, &
                       lat1=lat1)
  ELSE
    CALL efso_norm_amd(ctx, nml, nij1, nlev, member, nv3d, fcst3d, fcer3d, xf3d=xf, xg3d=xg, xa3d=xa)
  END IF
  ! das_efso, then print_obsense
  djdy = 0.0d0
  CALL das_efso_amd(ctx, t, nij1, nlev, member, nv3d, rig1, rjg1, rlev, hgt1, fcst3d, fcer3d, nterm, term_of_var, member, nobs, &
                    ya, dep, djdy, obsense)
  CALL print_obsense_amd(ctx, nterm, nobs, obsense, elm, typ, olat, uid, nobtype, otl, oel, latbound=r(11), nobs_sense=cnt, &
                         sumsense=ssum, nneg=neg)
  rc = letkf_ctx_destroy(ctx)

  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) fcst3d
  WRITE (u) fcer3d
  WRITE (u) obsense
  WRITE (u) ssum
  WRITE (u) cnt
  WRITE (u) neg
  CLOSE (u)

CONTAINS

  FUNCTION up(host, nbytes) RESULT(d)
    TYPE(c_ptr), INTENT(IN) :: host
    INTEGER(c_size_t), INTENT(IN) :: nbytes
    TYPE(c_ptr) :: d
    IF (hipMalloc(d, MAX(nbytes, 8_c_size_t)) /= 0) STOP 5
    IF (hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice) /= 0) STOP 5
  END FUNCTION up

END PROGRAM efso_norm_driver
