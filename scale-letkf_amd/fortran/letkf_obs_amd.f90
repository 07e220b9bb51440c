!===============================================================================
! letkf_obs_amd.f90 -- set_letkf_obs on the MI355X: the Fortran routine a host CALLs instead of the reference's
!   CALL set_letkf_obs                                 scale/letkf/letkf.f90:142, scale/letkf/letkf_obs.f90:142-1185
! for one subdomain (nprocs_d = 1).  The observation files (read_obs_all) and obsda (obsope) are the host's; everything from
! the pre-processing of the files (:268-305) to the assembly of obsda_sort (:1036-1100) runs on the device through
! letkf_set_obs_dev (include/letkf_amd.h section 9), and the table it builds STAYS there: the letkf_obs_tables_dev this
! routine returns goes straight into CALL das_letkf_amd(ctx, nml, tabd, ...) (letkf_tools_amd.f90), nothing is uploaded again.
! As the reference does to obs(:) and obsda, elm / dat / err of the files come back pre-processed, qc with the QC flags and
! ensval as perturbations.  Prints at LOG_LEVEL >= 1 the departure statistics (:639-646, monit_dep / monit_print of
! common_obs_scale.f90:1851-1948) and the per-type observation counts (:1161-1178).  A non-zero return code STOPs.
!===============================================================================
MODULE letkf_obs_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_tools_amd
  IMPLICIT NONE
  PRIVATE
  PUBLIC :: set_letkf_obs_amd, letkf_obs_nml

  INTEGER, PARAMETER :: r_size = c_double
  INTEGER, PARAMETER :: nid_obs = 16
  ! common_obs_scale.f90:74-77, :79-81, :85-92
  INTEGER(c_int32_t), PARAMETER :: elem_uid(nid_obs) = (/2819, 2820, 3073, 3074, 3330, 3331, 14593, 19999, 4001, 4004, 4002, &
                                                         4003, 8800, 99991, 99992, 99993/)
  CHARACTER(3), PARAMETER :: obelmlist(nid_obs) = (/'  U', '  V', '  T', ' Tv', '  Q', ' RH', ' PS', 'PRC', 'REF', 'RE0', ' Vr', &
                                                    'PRH', 'H08', 'TCX', 'TCY', 'TCP'/)
  CHARACTER(6), PARAMETER :: obtypelist(24) = (/'ADPUPA', 'AIRCAR', 'AIRCFT', 'SATWND', 'PROFLR', 'VADWND', 'SATEMP', 'ADPSFC', &
                                                'SFCSHP', 'SFCBOG', 'SPSSMI', 'SYNDAT', 'ERS1DA', 'GOESND', 'QKSWND', 'MSONET', &
                                                'GPSIPW', 'RASSDA', 'WDSATR', 'ASCATW', 'TMPAPR', 'PHARAD', 'H08IRB', 'TCVITL'/)

  ! namelist values set_letkf_obs reads (common_nml.f90), filled once per run like letkf_das_nml
  TYPE :: letkf_obs_nml
    INTEGER :: nobtype = 24
    REAL(r_size), ALLOCATABLE :: hori_local(:), vert_local(:)                   ! HORI_LOCAL, VERT_LOCAL (nobtype)
    REAL(r_size), ALLOCATABLE :: obs_sort_grid_spacing(:), obs_min_spacing(:)   ! OBS_SORT_GRID_SPACING, OBS_MIN_SPACING
    INTEGER, ALLOCATABLE :: max_nobs_per_grid(:)                                ! MAX_NOBS_PER_GRID
    INTEGER, ALLOCATABLE :: ctype_merge(:, :)             ! (nid_obs, nobtype), as letkf_das_nml%ctype_merge (unallocated: none)
    LOGICAL :: use_obserr_radar_ref = .FALSE., use_obserr_radar_vr = .FALSE.
    REAL(r_size) :: obserr_radar_ref = 5.0d0, obserr_radar_vr = 3.0d0
    REAL(r_size) :: min_radar_ref_dbz = 0.0d0, low_ref_shift = 0.0d0
    REAL(r_size) :: hori_local_radar_obsnoref = -1.0d0, hori_local_radar_vr = -1.0d0, vert_local_radar_vr = -1.0d0  ! < 0: type 22's
    REAL(r_size) :: dx = 0.0d0, dy = 0.0d0, vert_local_rain_base = 85000.0d0
    INTEGER :: nlon = 0, nlat = 0, ihalo = 2, jhalo = 2
    INTEGER :: max_nobs_per_grid_criterion = 1
    INTEGER :: log_level = 1                               ! LOG_LEVEL
    TYPE(letkf_qc_params) :: qc                            ! departure + QC (member, det_run, radar and gross-error settings, -DH08)
  END TYPE letkf_obs_nml

CONTAINS

  ! elm, typ, lev, dat, err, ri, rj: the OBS_IN_NUM files flattened, file f owns rows off(f)+1 .. off(f+1) (off(1) = 0).
  ! obsda: set, idx (1-based file and row), qc, ensval(nensobs, nobs) (nensobs = MEMBER (+1 with DET_RUN)); -DH08 builds
  ! (onml%qc%h08 = 1) pass obsda%lev and obsda%val2.  monit_*: the departure statistics per element (optional outputs).
  SUBROUTINE set_letkf_obs_amd(ctx, onml, nfile, off, elm, typ, lev, dat, err, ri, rj, nobs, set, idx, qc, ensval, tabd, &
                               obsda_lev, obsda_val2, monit_nobs, monit_bias, monit_rmse)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_obs_nml), INTENT(IN) :: onml
    INTEGER, INTENT(IN) :: nfile, nobs
    INTEGER(c_int64_t), INTENT(IN), TARGET :: off(nfile + 1)
    INTEGER(c_int32_t), INTENT(INOUT), TARGET :: elm(*)
    INTEGER(c_int32_t), INTENT(IN), TARGET :: typ(*)
    REAL(r_size), INTENT(IN), TARGET :: lev(*), ri(*), rj(*)
    REAL(r_size), INTENT(INOUT), TARGET :: dat(*), err(*)
    INTEGER(c_int32_t), INTENT(IN), TARGET :: set(nobs), idx(nobs)
    INTEGER(c_int32_t), INTENT(INOUT), TARGET :: qc(nobs)
    REAL(r_size), INTENT(INOUT), TARGET :: ensval(:, :)
    TYPE(letkf_obs_tables_dev), INTENT(INOUT) :: tabd
    REAL(r_size), INTENT(IN), OPTIONAL, TARGET :: obsda_lev(nobs)
    REAL(r_size), INTENT(INOUT), OPTIONAL, TARGET :: obsda_val2(nobs)
    INTEGER, INTENT(OUT), OPTIONAL :: monit_nobs(nid_obs)
    REAL(r_size), INTENT(OUT), OPTIONAL :: monit_bias(nid_obs), monit_rmse(nid_obs)

    TYPE(letkf_setobs_params) :: p
    TYPE(letkf_qc_params) :: q
    TYPE(letkf_obs_file_rows) :: f
    TYPE(letkf_obs_table_info) :: ti
    INTEGER(c_int64_t), ALLOCATABLE, TARGET :: off64(:)
    REAL(r_size), ALLOCATABLE, TARGET :: hl(:), vl(:), spc(:), msp(:)
    INTEGER(c_int32_t), ALLOCATABLE, TARGET :: mx(:), merge32(:, :), ac_ext(:)
    INTEGER(c_int32_t), POINTER :: ip(:)
    REAL(r_size), POINTER :: rp(:)
    INTEGER(c_int32_t), TARGET :: mnobs(nid_obs)
    REAL(r_size), TARGET :: mbias(nid_obs), mrmse(nid_obs)
    TYPE(c_ptr) :: d_elm, d_typ, d_lev, d_dat, d_err, d_ri, d_rj, d_set, d_idx, d_qc, d_ens, d_olev, d_val2, d_mn, d_mb, d_mr
    INTEGER(c_size_t) :: nr, nb
    INTEGER :: nt, nc, ic, kld, tot_ext, prev
    INTEGER(c_int) :: rc

    CALL letkf_obs_tables_dev_free(tabd)
    nt = onml%nobtype
    nr = INT(off(nfile + 1), c_size_t)
    kld = SIZE(ensval, 1)
    IF (nobs > 0 .AND. SIZE(ensval, 2) < nobs) CALL fail('ensval has fewer columns than obsda rows')
    ! ---- namelist -> letkf_setobs_params (the radar values resolved as common_nml.f90:772-780 does)
    ALLOCATE (hl(nt), vl(nt), spc(nt), msp(nt), mx(nt), merge32(nid_obs, nt), off64(nfile + 1))
    hl = onml%hori_local(1:nt); vl = onml%vert_local(1:nt); spc = onml%obs_sort_grid_spacing(1:nt)
    msp = onml%obs_min_spacing(1:nt); mx = onml%max_nobs_per_grid(1:nt); off64 = off
    merge32 = 0
    IF (ALLOCATED(onml%ctype_merge)) merge32 = onml%ctype_merge
    p%nobtype = nt
    p%use_obserr_radar_ref = MERGE(1, 0, onml%use_obserr_radar_ref); p%use_obserr_radar_vr = MERGE(1, 0, onml%use_obserr_radar_vr)
    p%nlon = onml%nlon; p%nlat = onml%nlat; p%ihalo = onml%ihalo; p%jhalo = onml%jhalo
    p%nprocs = 1; p%prc_num_x = 1; p%myrank = 0; p%fix_ij_obsgrd = 0; p%criterion = onml%max_nobs_per_grid_criterion
    p%min_radar_ref_dbz = onml%min_radar_ref_dbz; p%low_ref_shift = onml%low_ref_shift
    p%obserr_radar_ref = onml%obserr_radar_ref; p%obserr_radar_vr = onml%obserr_radar_vr
    p%hori_local_radar_obsnoref = MERGE(onml%hori_local(22), onml%hori_local_radar_obsnoref, onml%hori_local_radar_obsnoref < 0.0d0)
    p%hori_local_radar_vr = MERGE(onml%hori_local(22), onml%hori_local_radar_vr, onml%hori_local_radar_vr < 0.0d0)
    p%vert_local_radar_vr = MERGE(onml%vert_local(22), onml%vert_local_radar_vr, onml%vert_local_radar_vr < 0.0d0)
    p%dx = onml%dx; p%dy = onml%dy; p%rain_base = onml%vert_local_rain_base
    p%hori_local = c_loc(hl); p%vert_local = c_loc(vl); p%obs_sort_grid_spacing = c_loc(spc); p%obs_min_spacing = c_loc(msp)
    p%max_nobs_per_grid = c_loc(mx); p%ctype_merge = c_loc(merge32)

    ! ---- the files and obsda on the device
    d_elm = up(c_loc(elm), 4_c_size_t*nr); d_typ = up(c_loc(typ), 4_c_size_t*nr); d_lev = up(c_loc(lev), 8_c_size_t*nr)
    d_dat = up(c_loc(dat), 8_c_size_t*nr); d_err = up(c_loc(err), 8_c_size_t*nr)
    d_ri = up(c_loc(ri), 8_c_size_t*nr); d_rj = up(c_loc(rj), 8_c_size_t*nr)
    f%nfile = nfile; f%reserved0 = 0; f%off = c_loc(off64)
    f%elm = d_elm; f%typ = d_typ; f%lev = d_lev; f%dat = d_dat; f%err = d_err; f%ri = d_ri; f%rj = d_rj
    nb = INT(nobs, c_size_t)
    d_set = up(c_loc(set), 4_c_size_t*nb); d_idx = up(c_loc(idx), 4_c_size_t*nb); d_qc = up(c_loc(qc), 4_c_size_t*nb)
    d_ens = up(c_loc(ensval), 8_c_size_t*kld*nb)
    q = onml%qc
    d_olev = c_null_ptr; d_val2 = c_null_ptr
    IF (PRESENT(obsda_lev)) d_olev = up(c_loc(obsda_lev), 8_c_size_t*nb)
    IF (PRESENT(obsda_val2)) d_val2 = up(c_loc(obsda_val2), 8_c_size_t*nb)
    q%h08_lev = d_olev; q%h08_val2 = d_val2

    ! ---- CALL set_letkf_obs
    CALL chk(letkf_set_obs_dev(ctx, p, q, f, INT(nobs, c_int64_t), d_set, d_idx, d_qc, d_ens, INT(kld, c_int64_t), tabd%handle), &
             'letkf_set_obs_dev')
    CALL chk(letkf_obs_table_info_get(tabd%handle, ti), 'letkf_obs_table_info_get')

    ! ---- departure statistics (:639-646): monit_dep over the local rows
    CALL chk(hipMalloc(d_mn, 4_c_size_t*nid_obs), 'hipMalloc'); CALL chk(hipMalloc(d_mb, 8_c_size_t*nid_obs), 'hipMalloc')
    CALL chk(hipMalloc(d_mr, 8_c_size_t*nid_obs), 'hipMalloc')
    CALL chk(letkf_monit_dep_dev(ctx, nid_obs, elem_uid, INT(nobs, c_int64_t), ti%row_elm, ti%val, d_qc, d_mn, d_mb, d_mr), &
             'letkf_monit_dep_dev')
    CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')
    CALL chk(hipMemcpy(c_loc(mnobs), d_mn, 4_c_size_t*nid_obs, hipMemcpyDeviceToHost), 'download monit')
    CALL chk(hipMemcpy(c_loc(mbias), d_mb, 8_c_size_t*nid_obs, hipMemcpyDeviceToHost), 'download monit')
    CALL chk(hipMemcpy(c_loc(mrmse), d_mr, 8_c_size_t*nid_obs, hipMemcpyDeviceToHost), 'download monit')
    IF (PRESENT(monit_nobs)) monit_nobs = mnobs
    IF (PRESENT(monit_bias)) monit_bias = mbias
    IF (PRESENT(monit_rmse)) monit_rmse = mrmse

    ! ---- what the reference leaves in obs(:) and obsda
    CALL chk(hipMemcpy(c_loc(elm), d_elm, 4_c_size_t*nr, hipMemcpyDeviceToHost), 'download elm')
    CALL chk(hipMemcpy(c_loc(dat), d_dat, 8_c_size_t*nr, hipMemcpyDeviceToHost), 'download dat')
    CALL chk(hipMemcpy(c_loc(err), d_err, 8_c_size_t*nr, hipMemcpyDeviceToHost), 'download err')
    CALL chk(hipMemcpy(c_loc(qc), d_qc, 4_c_size_t*nb, hipMemcpyDeviceToHost), 'download qc')
    CALL chk(hipMemcpy(c_loc(ensval), d_ens, 8_c_size_t*kld*nb, hipMemcpyDeviceToHost), 'download ensval')
    IF (PRESENT(obsda_val2)) CALL chk(hipMemcpy(c_loc(obsda_val2), d_val2, 8_c_size_t*nb, hipMemcpyDeviceToHost), 'download val2')

    ! ---- the small host tables of tabd (letkf_obs.f90:35-72)
    nc = ti%nctype
    tabd%host%nctype = nc; tabd%host%nobstotal = INT(ti%nobstotal); tabd%host%nensobs = kld
    ALLOCATE (tabd%host%elm_ctype(nc), tabd%host%elm_u_ctype(nc), tabd%host%typ_ctype(nc), tabd%host%uid_varlocal_ctype(nc), &
              tabd%host%max_nobs_ctype(nc), tabd%host%hori_loc_ctype(nc), tabd%host%vert_loc_ctype(nc))
    IF (nc > 0) THEN
      CALL c_f_pointer(ti%elm_ctype, ip, (/nc/)); tabd%host%elm_ctype = ip
      CALL c_f_pointer(ti%elm_u_ctype, ip, (/nc/)); tabd%host%elm_u_ctype = ip
      CALL c_f_pointer(ti%typ_ctype, ip, (/nc/)); tabd%host%typ_ctype = ip
      CALL c_f_pointer(ti%hori_loc_ctype, rp, (/nc/)); tabd%host%hori_loc_ctype = rp
      CALL c_f_pointer(ti%vert_loc_ctype, rp, (/nc/)); tabd%host%vert_loc_ctype = rp
    END IF
    DO ic = 1, nc
      tabd%host%uid_varlocal_ctype(ic) = uid_obs_varlocal(tabd%host%elm_ctype(ic))
      tabd%host%max_nobs_ctype(ic) = onml%max_nobs_per_grid(tabd%host%typ_ctype(ic))
    END DO

    ! ---- prints at the reference's LOG_LEVEL
    IF (onml%log_level >= 1) THEN
      WRITE (6, *)
      WRITE (6, '(A,I6,A)') 'OBSERVATIONAL DEPARTURE STATISTICS (IN THIS SUBDOMAIN #', 0, '):'
      CALL monit_print(mnobs, mbias, mrmse)
      ALLOCATE (ac_ext(MAX(ti%nacx, 1_c_int64_t)))
      CALL chk(letkf_obs_table_download(ctx, tabd%handle, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr, &
                                        c_null_ptr, c_null_ptr, c_loc(ac_ext)), 'letkf_obs_table_download')
      CALL c_f_pointer(ti%tot_g, ip, (/2*MAX(nc, 1)/))
      WRITE (6, *)
      WRITE (6, '(A,I6,A)') 'OBSERVATION COUNTS (GLOABL AND IN THIS SUBDOMAIN #', 0, '):'
      WRITE (6, '(A)') '====================================================================='
      WRITE (6, '(A)') 'TYPE   VAR      GLOBAL     GLOBAL  SUBDOMAIN  SUBDOMAIN EXT_SUBDOMAIN'
      WRITE (6, '(A)') '             before QC   after QC  before QC   after QC      after QC'
      WRITE (6, '(A)') '---------------------------------------------------------------------'
      prev = 0
      DO ic = 1, nc
        ! tot_ext: the ctype's rows of obsda_sort = end of its ac_ext table minus the end of the previous one (cumulative)
        CALL ctype_end(ti, ic, ac_ext, tot_ext)
        WRITE (6, '(A6,1x,A3,1x,4I11,I14)') obtypelist(tabd%host%typ_ctype(ic)), obelmlist(tabd%host%elm_u_ctype(ic)), &
              ip(2*ic - 1), ip(2*ic), ip(2*ic - 1), ip(2*ic), tot_ext - prev
        prev = tot_ext
      END DO
      WRITE (6, '(A)') '---------------------------------------------------------------------'
      WRITE (6, '(A6,5x,4I11,I14)') 'TOTAL ', SUM(ip(1:2*nc:2)), SUM(ip(2:2*nc:2)), SUM(ip(1:2*nc:2)), SUM(ip(2:2*nc:2)), &
                                    tabd%host%nobstotal
      WRITE (6, '(A)') '====================================================================='
    END IF
    CALL free_all((/d_elm, d_typ, d_lev, d_dat, d_err, d_ri, d_rj, d_set, d_idx, d_qc, d_ens, d_mn, d_mb, d_mr/))
    IF (c_associated(d_olev)) rc = hipFree(d_olev)
    IF (c_associated(d_val2)) rc = hipFree(d_val2)
  END SUBROUTINE set_letkf_obs_amd

  ! entry (ngrdext_i, ngrdext_j) of ctype ic's ac_ext table: the rows of obsda_sort up to the end of ctype ic
  SUBROUTINE ctype_end(ti, ic, ac_ext, v)
    TYPE(letkf_obs_table_info), INTENT(IN) :: ti
    INTEGER, INTENT(IN) :: ic
    INTEGER(c_int32_t), INTENT(IN) :: ac_ext(:)
    INTEGER, INTENT(OUT) :: v
    INTEGER(c_int32_t), POINTER :: ei(:), ej(:)
    INTEGER(c_int64_t), POINTER :: ao(:)
    CALL c_f_pointer(ti%ngrdext_i, ei, (/ti%nctype/))
    CALL c_f_pointer(ti%ngrdext_j, ej, (/ti%nctype/))
    CALL c_f_pointer(ti%ac_off, ao, (/ti%nctype/))
    v = ac_ext(ao(ic) + INT(ei(ic) + 1, c_int64_t)*ej(ic))
  END SUBROUTINE ctype_end

  ! common_obs_scale.f90:215-243
  PURE FUNCTION uid_obs_varlocal(id) RESULT(u)
    INTEGER, INTENT(IN) :: id
    INTEGER :: u
    SELECT CASE (id)
    CASE (2819, 2820); u = 1
    CASE (3073, 3074); u = 2
    CASE (3330, 3331); u = 3
    CASE (14593); u = 4
    CASE (19999); u = 5
    CASE (99991, 99992, 99993); u = 6
    CASE (4001, 4004, 4003); u = 7
    CASE (4002); u = 8
    CASE (8800); u = 9
    CASE DEFAULT; u = -1
    END SELECT
  END FUNCTION uid_obs_varlocal

  ! common_obs_scale.f90:1899-1948 (Tv and RE0 are not shown)
  SUBROUTINE monit_print(nobs, bias, rmse)
    INTEGER(c_int32_t), INTENT(IN) :: nobs(nid_obs)
    REAL(r_size), INTENT(IN) :: bias(nid_obs), rmse(nid_obs)
    CHARACTER(12) :: var_show(nid_obs), nobs_show(nid_obs), bias_show(nid_obs), rmse_show(nid_obs)
    CHARACTER(4) :: nstr
    INTEGER :: i, n
    n = 0
    DO i = 1, nid_obs
      IF (i /= 4 .AND. i /= 10) THEN
        n = n + 1
        WRITE (var_show(n), '(A12)') obelmlist(i)
        WRITE (nobs_show(n), '(I12)') nobs(i)
        IF (nobs(i) > 0) THEN
          WRITE (bias_show(n), '(ES12.3)') bias(i)
          WRITE (rmse_show(n), '(ES12.3)') rmse(i)
        ELSE
          WRITE (bias_show(n), '(A12)') 'N/A'
          WRITE (rmse_show(n), '(A12)') 'N/A'
        END IF
      END IF
    END DO
    WRITE (nstr, '(I4)') n
    WRITE (6, '(A,'//TRIM(nstr)//"('============'))") '======'
    WRITE (6, '(6x,'//TRIM(nstr)//'A)') var_show(1:n)
    WRITE (6, '(A,'//TRIM(nstr)//"('------------'))") '------'
    WRITE (6, '(A,'//TRIM(nstr)//'A)') 'BIAS  ', bias_show(1:n)
    WRITE (6, '(A,'//TRIM(nstr)//'A)') 'RMSE  ', rmse_show(1:n)
    WRITE (6, '(A,'//TRIM(nstr)//'A)') 'NUMBER', nobs_show(1:n)
    WRITE (6, '(A,'//TRIM(nstr)//"('============'))") '======'
  END SUBROUTINE monit_print

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
      rc = hipFree(ptrs(i))
    END DO
  END SUBROUTINE free_all

  SUBROUTINE chk(rc, what)
    INTEGER(c_int), INTENT(IN) :: rc
    CHARACTER(*), INTENT(IN) :: what
    IF (rc /= 0) THEN
      WRITE (6, '(A,I6,2A)') 'set_letkf_obs_amd: error', rc, ' in ', what
      STOP 5
    END IF
  END SUBROUTINE chk

  SUBROUTINE fail(what)
    CHARACTER(*), INTENT(IN) :: what
    WRITE (6, '(2A)') 'set_letkf_obs_amd: ', what
    STOP 6
  END SUBROUTINE fail

END MODULE letkf_obs_amd
