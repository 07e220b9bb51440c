!===============================================================================
! efso_tools_amd.f90 -- the two ends of EFSO (scale/letkf/efso.f90) on the MI355X, the routines a maintainer CALLs instead
! of the reference's (include/letkf_amd.h section 13):
!   efso.f90:100-117 + CALL lnorm(fcst3d,fcst2d,fcer3d,fcer2d)   efso_norm_amd      (letkf_efso_norm_dev)
!   CALL print_obsense                                            print_obsense_amd  (letkf_efso_summary_dev + its WRITEs)
! Between them das_efso_amd (letkf_tools_amd.f90) computes obsense.  Host arrays in, host arrays out; the file I/O
! (read_ens_mpi, read_grd4, write_obs2) and the MPI_REDUCE of obsense over ranks stay with the caller.
! SCALE's build has nv2d = 0, so fcst2d / fcer2d and lnorm's ps term have no counterpart.  The layer weight sqrt(dp/ps)
! comes from the forecast-mean pressure by the half-level rule of the header (or from wlev), not from GFS's sigma
! coordinates.
!===============================================================================
MODULE efso_tools_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  IMPLICIT NONE
  PRIVATE
  PUBLIC :: efso_norm_amd, print_obsense_amd, efso_norm_nml

  INTEGER, PARAMETER :: r_size = c_double

  ! efso_nml.f90's EFSOPRM (target region, moist weight) and lnorm's constants; slots 1-based as common_scale.f90
  TYPE :: efso_norm_nml
    REAL(r_size) :: wmoist = 0.0d0
    REAL(r_size) :: tar_minlon = 0.0d0, tar_maxlon = 360.0d0, tar_minlat = -90.0d0, tar_maxlat = 90.0d0
    INTEGER :: tar_minlev = 1, tar_maxlev = 64
    REAL(r_size) :: cp = 1004.64d0, tref = 280.0d0, hvap = 2.501d6   ! CONST_CPdry, lnorm's tref, CONST_LHV0
    INTEGER :: iv3d_u = 1, iv3d_v = 2, iv3d_t = 4, iv3d_p = 5, iv3d_q = 6
  END TYPE efso_norm_nml

CONTAINS

  ! lnorm in SCALE's frame: fcst3d(nij1,nlev,nbv,nv3d) INOUT, total fields in, C^1/2 X^f out; fcer3d(nij1,nlev,nv3d)
  ! INOUT, C^1/2 times the forecast error.  With xf3d, xg3d and xa3d (the mean forecasts from the analysis and from the
  ! guess, and the verifying analysis) fcer3d is first assembled as efso.f90:100-117 does; otherwise it holds the error.
  ! wg1(nij1): area weight (absent = 1); lon1 / lat1(nij1): the target box's coordinates (absent = no box); wlev(nij1,nlev):
  ! dp/ps (absent = from the mean pressure); fmean3d(nij1,nlev,nv3d): the forecast mean, written when present.
  SUBROUTINE efso_norm_amd(ctx, nml, nij1, nlev, nbv, nv3d, fcst3d, fcer3d, xf3d, xg3d, xa3d, wg1, lon1, lat1, wlev, fmean3d)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(efso_norm_nml), INTENT(IN) :: nml
    INTEGER, INTENT(IN) :: nij1, nlev, nbv, nv3d
    REAL(r_size), INTENT(INOUT), TARGET :: fcst3d(nij1, nlev, nbv, nv3d), fcer3d(nij1, nlev, nv3d)
    REAL(r_size), INTENT(IN), TARGET, OPTIONAL :: xf3d(nij1, nlev, nv3d), xg3d(nij1, nlev, nv3d), xa3d(nij1, nlev, nv3d)
    REAL(r_size), INTENT(IN), TARGET, OPTIONAL :: wg1(nij1), lon1(nij1), lat1(nij1), wlev(nij1, nlev)
    REAL(r_size), INTENT(OUT), TARGET, OPTIONAL :: fmean3d(nij1, nlev, nv3d)
    TYPE(letkf_efso_norm_params) :: p
    TYPE(c_ptr) :: d_f, d_e, d_xf, d_xg, d_xa, d_wg, d_lon, d_lat, d_wl, d_fm
    INTEGER(c_int64_t) :: npts
    INTEGER(c_size_t) :: nbf, nbe, nbh

    npts = INT(nij1, c_int64_t)*nlev
    nbf = 8_c_size_t*npts*nbv*nv3d
    nbe = 8_c_size_t*npts*nv3d
    nbh = 8_c_size_t*nij1
    p%k = nbv
    p%nv = nv3d
    p%iv_u = nml%iv3d_u - 1
    p%iv_v = nml%iv3d_v - 1
    p%iv_t = nml%iv3d_t - 1
    p%iv_q = nml%iv3d_q - 1
    p%iv_p = nml%iv3d_p - 1
    p%tar_minlev = nml%tar_minlev
    p%tar_maxlev = nml%tar_maxlev
    p%cp = nml%cp
    p%tref = nml%tref
    p%hvap = nml%hvap
    p%wmoist = nml%wmoist
    p%tar_minlon = nml%tar_minlon
    p%tar_maxlon = nml%tar_maxlon
    p%tar_minlat = nml%tar_minlat
    p%tar_maxlat = nml%tar_maxlat
    d_f = up(c_loc(fcst3d), nbf)
    d_e = up(c_loc(fcer3d), nbe)
    d_xf = c_null_ptr; d_xg = c_null_ptr; d_xa = c_null_ptr
    d_wg = c_null_ptr; d_lon = c_null_ptr; d_lat = c_null_ptr; d_wl = c_null_ptr; d_fm = c_null_ptr
    IF (PRESENT(xf3d) .AND. PRESENT(xg3d) .AND. PRESENT(xa3d)) THEN
      d_xf = up(c_loc(xf3d), nbe)
      d_xg = up(c_loc(xg3d), nbe)
      d_xa = up(c_loc(xa3d), nbe)
    END IF
    IF (PRESENT(wg1)) d_wg = up(c_loc(wg1), nbh)
    IF (PRESENT(lon1) .AND. PRESENT(lat1)) THEN
      d_lon = up(c_loc(lon1), nbh)
      d_lat = up(c_loc(lat1), nbh)
    END IF
    IF (PRESENT(wlev)) d_wl = up(c_loc(wlev), 8_c_size_t*npts)
    IF (PRESENT(fmean3d)) CALL chk(hipMalloc(d_fm, MAX(nbe, 8_c_size_t)), 'hipMalloc fmean')
    CALL chk(letkf_efso_norm_dev(ctx, p, INT(nij1, c_int64_t), INT(nlev, c_int32_t), d_f, 1_c_int64_t, npts, npts*nbv, d_fm, &
                                 d_e, 1_c_int64_t, npts, d_xf, d_xg, d_xa, d_wl, d_wg, d_lon, d_lat), 'letkf_efso_norm_dev')
    CALL chk(letkf_ctx_synchronize(ctx), 'letkf_ctx_synchronize')
    CALL chk(hipMemcpy(c_loc(fcst3d), d_f, nbf, hipMemcpyDeviceToHost), 'download fcst3d')
    CALL chk(hipMemcpy(c_loc(fcer3d), d_e, nbe, hipMemcpyDeviceToHost), 'download fcer3d')
    IF (PRESENT(fmean3d)) CALL chk(hipMemcpy(c_loc(fmean3d), d_fm, nbe, hipMemcpyDeviceToHost), 'download fmean3d')
    CALL free_all([d_f, d_e, d_xf, d_xg, d_xa, d_wg, d_lon, d_lat, d_wl, d_fm])
  END SUBROUTINE efso_norm_amd

  ! print_obsense (efso_tools.f90:197-290, without its write_obs2 files): the table per observation type x region x element
  ! of obsense(nterm, nobs) (das_efso_amd's), WRITten to unit (default 6) with the reference's formats for term 1 (KE).
  ! elm / typ: NINT(obselm) / NINT(obstyp); lat: obslat; qc (optional): rows with qc /= 0 are skipped; elem_uid(nid): the
  ! element ids in the order of obelmlist(nid) (uid_obs); obtypelist(nobtype); latbound (default 20).  The tables of every
  ! term come back in nobs_sense(nid, nobtype+1, 3), sumsense(nid, nobtype+1, 3, nterm), nneg (same shape), regions
  ! NH, TR, SH.  Nothing is printed when nobs = 0, as the reference.
  SUBROUTINE print_obsense_amd(ctx, nterm, nobs, obsense, elm, typ, lat, elem_uid, nobtype, obtypelist, obelmlist, latbound, qc, &
                               unit, nobs_sense, sumsense, nneg)
    TYPE(c_ptr), INTENT(IN) :: ctx
    INTEGER, INTENT(IN) :: nterm, nobs, nobtype
    REAL(r_size), INTENT(IN), TARGET :: obsense(nterm, nobs), lat(nobs)
    INTEGER(c_int32_t), INTENT(IN), TARGET :: elm(nobs), typ(nobs)
    INTEGER(c_int32_t), INTENT(IN), TARGET, CONTIGUOUS :: elem_uid(:)
    CHARACTER(len=*), INTENT(IN) :: obtypelist(nobtype), obelmlist(:)
    REAL(r_size), INTENT(IN), OPTIONAL :: latbound
    INTEGER(c_int32_t), INTENT(IN), TARGET, OPTIONAL :: qc(nobs)
    INTEGER, INTENT(IN), OPTIONAL :: unit
    INTEGER(c_int32_t), INTENT(OUT), OPTIONAL :: nobs_sense(SIZE(elem_uid), nobtype + 1, 3)
    REAL(r_size), INTENT(OUT), OPTIONAL :: sumsense(SIZE(elem_uid), nobtype + 1, 3, nterm)
    INTEGER(c_int32_t), INTENT(OUT), OPTIONAL :: nneg(SIZE(elem_uid), nobtype + 1, 3, nterm)
    INTEGER, PARAMETER :: nreg = 3
    CHARACTER(len=2), PARAMETER :: charreg(nreg) = ['NH', 'TR', 'SH']
    INTEGER(c_int32_t), TARGET :: cnt(SIZE(elem_uid), nobtype + 1, nreg), neg(SIZE(elem_uid), nobtype + 1, nreg, nterm)
    REAL(r_size), TARGET :: ssum(SIZE(elem_uid), nobtype + 1, nreg, nterm)
    TYPE(c_ptr) :: d_ob, d_elm, d_typ, d_lat, d_qc, d_cnt, d_sum, d_neg
    INTEGER(c_size_t) :: nbc, nbs
    INTEGER :: u, nid, otype, ireg, oid, nobs_t
    REAL(r_size) :: lb, sumsense_t, rate_t
    CHARACTER(len=6) :: charotype

    nid = SIZE(elem_uid)
    u = 6
    IF (PRESENT(unit)) u = unit
    lb = 20.0d0
    IF (PRESENT(latbound)) lb = latbound
    nbc = 4_c_size_t*nid*(nobtype + 1)*nreg
    nbs = 8_c_size_t*nid*(nobtype + 1)*nreg*nterm
    d_ob = up(c_loc(obsense), 8_c_size_t*nterm*nobs)
    d_elm = up(c_loc(elm), 4_c_size_t*nobs)
    d_typ = up(c_loc(typ), 4_c_size_t*nobs)
    d_lat = up(c_loc(lat), 8_c_size_t*nobs)
    d_qc = c_null_ptr
    IF (PRESENT(qc)) d_qc = up(c_loc(qc), 4_c_size_t*nobs)
    CALL chk(hipMalloc(d_cnt, nbc), 'hipMalloc count')
    CALL chk(hipMalloc(d_sum, nbs), 'hipMalloc sum')
    CALL chk(hipMalloc(d_neg, nbs/2), 'hipMalloc nneg')
    CALL chk(letkf_efso_summary_dev(ctx, INT(nterm, c_int32_t), INT(nobs, c_int64_t), d_ob, d_elm, d_typ, d_lat, d_qc, &
                                    INT(nid, c_int32_t), c_loc(elem_uid), INT(nobtype, c_int32_t), lb, d_cnt, d_sum, d_neg), &
             'letkf_efso_summary_dev')
    CALL chk(letkf_ctx_synchronize(ctx), 'letkf_ctx_synchronize')
    CALL chk(hipMemcpy(c_loc(cnt), d_cnt, nbc, hipMemcpyDeviceToHost), 'download count')
    CALL chk(hipMemcpy(c_loc(ssum), d_sum, nbs, hipMemcpyDeviceToHost), 'download sum')
    CALL chk(hipMemcpy(c_loc(neg), d_neg, nbs/2, hipMemcpyDeviceToHost), 'download nneg')
    CALL free_all([d_ob, d_elm, d_typ, d_lat, d_qc, d_cnt, d_sum, d_neg])
    IF (PRESENT(nobs_sense)) nobs_sense = cnt
    IF (PRESENT(sumsense)) sumsense = ssum
    IF (PRESENT(nneg)) nneg = neg
    IF (nobs == 0) RETURN

    WRITE (u, '(A)') '============================================'
    WRITE (u, '(A,I10)') ' TOTAL NUMBER OF OBSERVATIONS:', nobs
    WRITE (u, '(A)') '============================================'
    WRITE (u, '(A)') '              nobs     dJ(KE)       +rate[%]'
    DO otype = 1, nobtype + 1
      IF (otype <= nobtype) THEN
        charotype = obtypelist(otype)
      ELSE
        charotype = 'OTHERS'
      END IF
      nobs_t = SUM(cnt(:, otype, :))
      IF (nobs_t > 0) THEN
        sumsense_t = 0.0d0                 ! SUM(sumsense(:,otype,:)) and SUM(rate(:,otype,:)), element order
        rate_t = 0.0d0
        DO ireg = 1, nreg
          DO oid = 1, nid
            sumsense_t = sumsense_t + ssum(oid, otype, ireg, 1)
            rate_t = rate_t + REAL(neg(oid, otype, ireg, 1), r_size)
          END DO
        END DO
        rate_t = rate_t/REAL(nobs_t, r_size)*100.0d0
        WRITE (u, '(A)') '--------------------------------------------'
        WRITE (u, '(A,1x,A,1x,I8,1x,E12.5,1x,F8.2)') charotype, ' TOTAL', nobs_t, sumsense_t, rate_t
      END IF
      DO ireg = 1, nreg
        DO oid = 1, nid
          IF (cnt(oid, otype, ireg) > 0) THEN
            rate_t = REAL(neg(oid, otype, ireg, 1), r_size)/REAL(cnt(oid, otype, ireg), r_size)*100.0d0
            WRITE (u, '(A,1x,A,1x,A,1x,I8,1x,E12.5,1x,F8.2)') charotype, charreg(ireg), obelmlist(oid), cnt(oid, otype, ireg), &
              ssum(oid, otype, ireg, 1), rate_t
          END IF
        END DO
      END DO
    END DO
    WRITE (u, '(A)') '============================================'
  END SUBROUTINE print_obsense_amd

  FUNCTION up(host, nbytes) RESULT(d)
    TYPE(c_ptr), INTENT(IN) :: host
    INTEGER(c_size_t), INTENT(IN) :: nbytes
    TYPE(c_ptr) :: d
    CALL chk(hipMalloc(d, MAX(nbytes, 8_c_size_t)), 'hipMalloc')
    IF (nbytes > 0) CALL chk(hipMemcpy(d, host, nbytes, hipMemcpyHostToDevice), 'hipMemcpy H2D')
  END FUNCTION up

  SUBROUTINE free_all(ptrs)
    TYPE(c_ptr), INTENT(IN) :: ptrs(:)
    INTEGER :: i
    INTEGER(c_int) :: rc
    DO i = 1, SIZE(ptrs)
      IF (c_associated(ptrs(i))) rc = hipFree(ptrs(i))
    END DO
  END SUBROUTINE free_all

  SUBROUTINE chk(rc, what)
    INTEGER(c_int), INTENT(IN) :: rc
    CHARACTER(*), INTENT(IN) :: what
    IF (rc /= 0) THEN
      WRITE (6, '(A,I6,2A)') 'efso_tools_amd: error', rc, ' in ', what
      STOP 5
    END IF
  END SUBROUTINE chk

END MODULE efso_tools_amd
