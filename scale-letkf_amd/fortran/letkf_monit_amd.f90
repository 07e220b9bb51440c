!===============================================================================
! letkf_monit_amd.f90 -- Fortran side of include/letkf_amd_monit.h: the departure monitor monit_obs on the device.  The
! BIND(C) mirrors of letkf_hist_state, letkf_monit_params and letkf_obsdep (fields in C order), the interfaces of the three
! entries, and the calls that stand where monit_obs stood: state_to_history_amd, monit_obs_amd and monit_print_amd
! (scale/common/common_obs_scale.f90:1370-1844 and :1899-1948).
!===============================================================================
MODULE letkf_monit_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  USE letkf_obsope_amd
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_MONIT_VERSION = 1
  INTEGER, PARAMETER :: nid_obs_monit = 16
  ! common_obs_scale.f90:74-81
  INTEGER(c_int32_t), PARAMETER :: elem_uid_monit(nid_obs_monit) = &
    (/2819, 2820, 3073, 3074, 3330, 3331, 14593, 19999, 4001, 4004, 4002, 4003, 8800, 99991, 99992, 99993/)
  CHARACTER(3), PARAMETER :: obelmlist(nid_obs_monit) = &
    (/'  U', '  V', '  T', ' Tv', '  Q', ' RH', ' PS', 'PRC', 'REF', 'RE0', ' Vr', 'PRH', 'H08', 'TCX', 'TCY', 'TCP'/)
  INTEGER, PARAMETER :: uid_tv_monit = 4, uid_re0_monit = 10

  TYPE, BIND(C) :: letkf_hist_state
    INTEGER(c_int32_t) :: nv3d
    INTEGER(c_int32_t) :: edge_fill                   ! bit 0 west, 1 east, 2 south, 3 north
    TYPE(c_ptr)        :: x                           ! dev
    INTEGER(c_int64_t) :: si, sj, sl, sv
    TYPE(c_ptr)        :: topo                        ! dev (nlon, nlat)
    TYPE(c_ptr)        :: cz                          ! HOST real64 (nlev)
    REAL(c_double)     :: ztop
  END TYPE letkf_hist_state

  TYPE, BIND(C) :: letkf_monit_params
    INTEGER(c_int32_t) :: step
    INTEGER(c_int32_t) :: departure_stat_radar
    INTEGER(c_int32_t) :: nid, reserved0
    TYPE(c_ptr)        :: elem_uid                    ! HOST int32 (nid)
    REAL(c_double)     :: t_range
    TYPE(c_ptr)        :: dif                         ! dev, per file row
  END TYPE letkf_monit_params

  TYPE, BIND(C) :: letkf_obsdep
    TYPE(c_ptr)        :: set, idx, qc                ! dev int32 (nn)
    TYPE(c_ptr)        :: omb, oma                    ! dev real64 (nn)
  END TYPE letkf_obsdep

  INTERFACE
    FUNCTION letkf_state_to_history_dev(ctx, s, layout, v3d, v2d) BIND(C, name='letkf_state_to_history_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_hist_state, letkf_obsope_fields
      TYPE(c_ptr), VALUE :: ctx, v3d, v2d
      TYPE(letkf_hist_state), INTENT(IN) :: s
      TYPE(letkf_obsope_fields), INTENT(IN) :: layout
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_monit_obs_dev(ctx, mp, op, files, f, nn, key, set, idx, rec, nobs, bias, rmse) &
        BIND(C, name='letkf_monit_obs_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t, letkf_monit_params, letkf_obsope_params, letkf_obs_file_rows, letkf_obsope_fields, &
                letkf_obsdep
      TYPE(c_ptr), VALUE :: ctx, key, set, idx, nobs, bias, rmse
      TYPE(letkf_monit_params), INTENT(IN) :: mp
      TYPE(letkf_obsope_params), INTENT(IN) :: op
      TYPE(letkf_obs_file_rows), INTENT(IN) :: files
      TYPE(letkf_obsope_fields), INTENT(IN) :: f
      INTEGER(c_int64_t), VALUE :: nn
      TYPE(letkf_obsdep), INTENT(IN) :: rec
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_monit_type(nid, elem_uid, departure_stat_radar, departure_stat_h08, monit_type) &
        BIND(C, name='letkf_monit_type') RESULT(rc)
      IMPORT :: c_int, c_int32_t
      INTEGER(c_int32_t), VALUE :: nid, departure_stat_radar, departure_stat_h08
      INTEGER(c_int32_t), INTENT(IN) :: elem_uid(*)
      INTEGER(c_int32_t), INTENT(OUT) :: monit_type(*)
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! state_to_history: the state `st` into member slot 0 of the history fields v3d / v2d (DEVICE) laid out as `layout` says.
  SUBROUTINE state_to_history_amd(ctx, st, layout, v3d, v2d, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_hist_state), INTENT(IN) :: st
    TYPE(letkf_obsope_fields), INTENT(IN) :: layout
    TYPE(c_ptr), INTENT(IN) :: v3d, v2d
    INTEGER, INTENT(OUT) :: ierr
    ierr = letkf_state_to_history_dev(ctx, st, layout, v3d, v2d)
  END SUBROUTINE state_to_history_amd

  ! monit_obs of step mprm%step over the rows key(1 .. nn) of obsda's set / idx (key = c_null_ptr: the first nn rows).
  ! nfile, off (HOST), elm .. rj, dat (DEVICE): the observation files as set_letkf_obs_amd left them.  rec: the obsdep
  ! records (DEVICE), written at step 1 and merged at step 2.  nobs, bias, rmse, monit_type: HOST (mprm%nid), as monit_obs
  ! returns them (the statistics come back with one synchronisation).
  SUBROUTINE monit_obs_amd(ctx, mprm, prm, nfile, off, elm, typ, lev, ri, rj, dat, fields, nn, key, set, idx, rec, &
                           nobs, bias, rmse, monit_type, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_monit_params), INTENT(IN) :: mprm
    TYPE(letkf_obsope_params), INTENT(IN) :: prm
    INTEGER, INTENT(IN) :: nfile
    INTEGER(c_int64_t), INTENT(IN), TARGET :: off(nfile + 1)
    TYPE(c_ptr), INTENT(IN) :: elm, typ, lev, ri, rj, dat
    TYPE(letkf_obsope_fields), INTENT(IN) :: fields
    INTEGER(c_int64_t), INTENT(IN) :: nn
    TYPE(c_ptr), INTENT(IN) :: key, set, idx
    TYPE(letkf_obsdep), INTENT(IN) :: rec
    INTEGER(c_int32_t), INTENT(OUT), TARGET :: nobs(mprm%nid)
    REAL(c_double), INTENT(OUT), TARGET :: bias(mprm%nid), rmse(mprm%nid)
    LOGICAL, INTENT(OUT) :: monit_type(mprm%nid)
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_obs_file_rows) :: files
    TYPE(c_ptr) :: d_n, d_b, d_r
    INTEGER(c_int32_t) :: mt(mprm%nid)
    INTEGER(c_int32_t), POINTER :: uid(:)
    INTEGER(c_int) :: rc
    INTEGER(c_size_t) :: nid

    nid = mprm%nid
    files%nfile = nfile; files%reserved0 = 0
    files%off = c_loc(off)
    files%elm = elm; files%typ = typ; files%lev = lev; files%ri = ri; files%rj = rj
    files%dat = dat; files%err = c_null_ptr                              ! (the monitor does not read err)
    ierr = hipMalloc(d_n, 4_c_size_t*nid); IF (ierr /= 0) RETURN
    ierr = hipMalloc(d_b, 8_c_size_t*nid); IF (ierr /= 0) RETURN
    ierr = hipMalloc(d_r, 8_c_size_t*nid); IF (ierr /= 0) RETURN
    ierr = letkf_monit_obs_dev(ctx, mprm, prm, files, fields, nn, key, set, idx, rec, d_n, d_b, d_r)
    IF (ierr == 0) ierr = letkf_ctx_synchronize(ctx)
    IF (ierr == 0) ierr = hipMemcpy(c_loc(nobs), d_n, 4_c_size_t*nid, hipMemcpyDeviceToHost)
    IF (ierr == 0) ierr = hipMemcpy(c_loc(bias), d_b, 8_c_size_t*nid, hipMemcpyDeviceToHost)
    IF (ierr == 0) ierr = hipMemcpy(c_loc(rmse), d_r, 8_c_size_t*nid, hipMemcpyDeviceToHost)
    rc = hipFree(d_n); rc = hipFree(d_b); rc = hipFree(d_r)
    IF (ierr /= 0) RETURN
    CALL c_f_pointer(mprm%elem_uid, uid, (/mprm%nid/))
    ierr = letkf_monit_type(mprm%nid, uid, mprm%departure_stat_radar, 0_c_int32_t, mt)
    monit_type = mt /= 0
  END SUBROUTINE monit_obs_amd

  ! monit_print, common_obs_scale.f90:1899-1948: the table of the elements with monit_type set, except Tv and RE0 (counted
  ! as T and REF).  For the reference's sixteen elements (obelmlist).
  SUBROUTINE monit_print_amd(nobs, bias, rmse, monit_type)
    INTEGER(c_int32_t), INTENT(IN) :: nobs(nid_obs_monit)
    REAL(c_double), INTENT(IN) :: bias(nid_obs_monit), rmse(nid_obs_monit)
    LOGICAL, INTENT(IN), OPTIONAL :: monit_type(nid_obs_monit)
    CHARACTER(12) :: var_show(nid_obs_monit), nobs_show(nid_obs_monit), bias_show(nid_obs_monit), rmse_show(nid_obs_monit)
    INTEGER :: i, n
    CHARACTER(4) :: nstr
    LOGICAL :: monit_type_(nid_obs_monit)

    monit_type_ = .TRUE.
    IF (PRESENT(monit_type)) monit_type_ = monit_type
    n = 0
    DO i = 1, nid_obs_monit
      IF (monit_type_(i) .AND. i /= uid_tv_monit .AND. i /= uid_re0_monit) THEN
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
  END SUBROUTINE monit_print_amd

END MODULE letkf_monit_amd
