!===============================================================================
! obsanal_driver.f90 -- a Fortran host calling das_letkf_obs_amd (letkf_tools_amd.f90): reads the search tables, the
! observation table and the targets from a case file written by tests/test_fortran_obsanal.py, uploads the tables (what
! set_letkf_obs_amd would leave on the device), makes the call (one letkf_das_obs_dev per target variable) and writes ya,
! ya_mean, dep_a and ya_table.
!   file (little endian, stream): int32 hdr(16); real64 r(10); then the arrays in the order read below
!===============================================================================
PROGRAM obsanal_driver
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_tools_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: hdr(16)
  REAL(c_double) :: r(10)
  INTEGER :: nctype, ngroup, kld, nobs, nacx, ngm, ntgt, nvar, lda, u, ios
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: gs(:), gm(:), vmode(:), mx(:), gi(:), gj(:), si(:), sj(:), ei(:), ej(:), ace(:)
  INTEGER(c_int32_t), ALLOCATABLE :: uid32(:), row32(:), elm32(:)
  INTEGER(c_int64_t), ALLOCATABLE, TARGET :: aco(:)
  REAL(c_double), ALLOCATABLE, TARGET :: hl(:), vl(:), vloc(:), ori(:), orj(:), olev(:), odat(:), oerr(:)
  REAL(c_double), ALLOCATABLE :: ensval(:, :), dep(:), ya_table(:, :), rlev(:), rz(:), infl(:), ya(:, :), ya_mean(:), dep_a(:)
  TYPE(letkf_search_tables) :: t
  TYPE(letkf_das_nml) :: nml
  TYPE(c_ptr) :: ctx
  CHARACTER(len=512) :: fin, fout
  INTEGER(c_int) :: rc

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) hdr
  READ (u) r
  nctype = hdr(1); ngroup = hdr(2); kld = hdr(8); nobs = hdr(9); nacx = hdr(10); ngm = hdr(11); ntgt = hdr(12); nvar = hdr(13)
  nml%member = hdr(6)
  nml%det_run = hdr(7) /= 0
  nml%relax_to_inflated_prior = hdr(14) /= 0
  nml%list_bytes = hdr(15)
  nml%infl_mul = r(6); nml%relax_alpha = r(7); nml%relax_alpha_spread = r(8); nml%q_update_top = r(9); nml%q_sprd_max = r(10)
  lda = nml%member + MERGE(1, 0, nml%det_run)
  ALLOCATE (gs(ngroup + 1), gm(ngm), vmode(nctype), mx(nctype), gi(nctype), gj(nctype), si(nctype), sj(nctype), ei(nctype), &
            ej(nctype), uid32(nctype), aco(nctype), ace(nacx), hl(nctype), vl(nctype), vloc(nctype), ori(nobs), orj(nobs), &
            olev(nobs), odat(nobs), oerr(nobs), ensval(kld, nobs), dep(nobs), ya_table(kld, nobs), row32(ntgt), elm32(ntgt), &
            rlev(ntgt), rz(ntgt), infl(ntgt), nml%var_local(nvar, 9), ya(lda, ntgt), ya_mean(ntgt), dep_a(ntgt))
  READ (u) gs, gm, vmode, mx, gi, gj, si, sj, ei, ej, uid32
  READ (u) aco
  READ (u) ace
  READ (u) hl, vl, vloc, ori, orj, olev, odat, oerr, ensval, dep, ya_table
  READ (u) row32, elm32
  READ (u) rlev, rz, infl, nml%var_local
  CLOSE (u)

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
  CALL das_letkf_obs_amd(ctx, nml, t, nctype, INT(uid32), kld, nobs, ensval, dep, ntgt, INT(row32), INT(elm32), ya, ya_mean, &
                         dep_a, ya_table, rlev_tgt=rlev, rz_tgt=rz, infl=infl)
  ! varloc is back as it was uploaded
  IF (hipMemcpy(c_loc(hl), t%varloc, 8_c_size_t*nctype, hipMemcpyDeviceToHost) /= 0) STOP 5
  IF (ANY(hl /= vloc)) STOP 7
  rc = letkf_ctx_destroy(ctx)

  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) ya
  WRITE (u) ya_mean
  WRITE (u) dep_a
  WRITE (u) ya_table
  CLOSE (u)

CONTAINS

  FUNCTION up(host, nbytes) RESULT(d)
    TYPE(c_ptr), INTENT(IN) :: host
    INTEGER(c_size_t), INTENT(IN) :: nbytes
    TYPE(c_ptr) :: d
    IF (hipMalloc(d, MAX(nbytes, 8_c_size_t)) /= 0) STOP 5
    IF (hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice) /= 0) STOP 5
  END FUNCTION up

END PROGRAM obsanal_driver
