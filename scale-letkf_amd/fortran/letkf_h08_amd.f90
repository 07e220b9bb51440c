!===============================================================================
! letkf_h08_amd.f90 -- Fortran side of include/letkf_amd_h08.h: Himawari-8 infrared radiances on the device.  The BIND(C) mirrors
! of letkf_h08_params and letkf_h08_profiles (fields in C order) and the interfaces of the seven entries of libletkf_amd_h08.so;
! letkf_obsope_fields is the operator's module's, letkf_obsfile_cols the record codec's.  The order of calls for a host
! (INTEGRATION.md): letkf_h08_decode_dev where read_obs_H08 stands, phys2ij, the first scan, the operator for all members, then
!   letkf_h08_select_dev     which profiles of the file the obsda rows of this call name (scale/obs/obsope_tools.f90:512-560)
!   letkf_h08_profiles_dev   stands where Trans_XtoY_H08 fills prs2d .. lsmask1d (scale/common/common_obs_scale.f90:2842-2875) and,
!                            with rttov_units, where SCALE_RTTOV_fwd fills RTTOV's profiles (scale/common/scale_H08_fwd.F90:518-632)
!   (the host's rttov_direct on the downloaded arrays; btall, btclr and trans uploaded)
!   letkf_h08_rows_dev       stands where Trans_XtoY_H08 finds the weighting function's peak (:2913-2966) and obsope_cal fills the
!                            obsda rows (obsope_tools.f90:594-634)
! and set_letkf_obs with h08 = 1.  Every level index is the model's, bottom up, unless top_down is set.
!===============================================================================
MODULE letkf_h08_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_obsope_amd
  USE letkf_obsfile_amd
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_H08_VERSION = 1
  INTEGER(c_int32_t), PARAMETER :: LETKF_H08_NCH = 10, LETKF_H08_ID = 8800, LETKF_H08_QC_BAD = 50

  TYPE, BIND(C) :: letkf_h08_params
    INTEGER(c_int32_t) :: nlev, nprof_file
    INTEGER(c_int32_t) :: top_down, stggrd, rttov_units, reject_land
    INTEGER(c_int32_t) :: use_obs23, finish, member, reserved0
    INTEGER(c_int32_t) :: ch_use(10)                                 ! H08_CH_USE
    REAL(c_double)     :: ri_off, rj_off                             ! rank_i * nlon, rank_j * nlat
    REAL(c_double)     :: rd, rv, q_ppmv, qmin, minq, cfrac_cnst
    REAL(c_double)     :: sub_lon, r_pol, r_sat, ell_tan, ell_ecc
    REAL(c_double)     :: cldsky_thrs, bris, brie, brjs, brje
  END TYPE letkf_h08_params

  TYPE, BIND(C) :: letkf_h08_profiles
    TYPE(c_ptr) :: lev3, sfc, cloud                                  ! dev real64
    TYPE(c_ptr) :: pflag                                             ! dev int32 (nsel)
  END TYPE letkf_h08_profiles

  INTERFACE
    FUNCTION letkf_h08_count(nbytes, nprof) BIND(C, name='letkf_h08_count') RESULT(rc)
      IMPORT :: c_int, c_int64_t
      INTEGER(c_int64_t), VALUE :: nbytes
      INTEGER(c_int64_t), INTENT(OUT) :: nprof
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_h08_bytes(nprof, nbytes) BIND(C, name='letkf_h08_bytes') RESULT(rc)
      IMPORT :: c_int, c_int64_t
      INTEGER(c_int64_t), VALUE :: nprof
      INTEGER(c_int64_t), INTENT(OUT) :: nbytes
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_h08_decode_dev(ctx, big_endian, image, nprof, obserr, cols, nbad) BIND(C, name='letkf_h08_decode_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t, c_double, letkf_obsfile_cols
      TYPE(c_ptr), VALUE :: ctx, image, nbad                         ! nbad: HOST int64 or c_null_ptr
      INTEGER(c_int32_t), VALUE :: big_endian
      INTEGER(c_int64_t), VALUE :: nprof
      REAL(c_double), INTENT(IN) :: obserr(10)                       ! OBSERR_H08
      TYPE(letkf_obsfile_cols), INTENT(IN) :: cols
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_h08_encode_dev(ctx, big_endian, nprof, cols, image) BIND(C, name='letkf_h08_encode_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t, letkf_obsfile_cols
      TYPE(c_ptr), VALUE :: ctx, image
      INTEGER(c_int32_t), VALUE :: big_endian
      INTEGER(c_int64_t), VALUE :: nprof
      TYPE(letkf_obsfile_cols), INTENT(IN) :: cols
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_h08_select_dev(ctx, set, idx, row0, nrows, h08_set, nprof_file, prof_list, slot_of_prof, nsel) &
        BIND(C, name='letkf_h08_select_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t
      TYPE(c_ptr), VALUE :: ctx, set, idx, prof_list, slot_of_prof
      INTEGER(c_int64_t), VALUE :: row0, nrows, nprof_file
      INTEGER(c_int32_t), VALUE :: h08_set
      INTEGER(c_int64_t), INTENT(OUT) :: nsel                        ! HOST: the entry's one read-back
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_h08_profiles_dev(ctx, p, f, nsel, prof_list, ri, rj, lon, lat, rotc, out) &
        BIND(C, name='letkf_h08_profiles_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t, letkf_h08_params, letkf_obsope_fields, letkf_h08_profiles
      TYPE(c_ptr), VALUE :: ctx, prof_list, ri, rj, lon, lat, rotc   ! rotc: dev (2, file profiles) or c_null_ptr
      TYPE(letkf_h08_params), INTENT(IN) :: p
      TYPE(letkf_obsope_fields), INTENT(IN) :: f
      INTEGER(c_int64_t), VALUE :: nsel
      TYPE(letkf_h08_profiles), INTENT(IN) :: out
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_h08_rows_dev(ctx, p, row0, nrows, set, idx, h08_set, slot_of_prof, nsel, nmem, m0, lev3, sfc, pflag, btall, &
                                btclr, trans, rig, rjg, qc_replace, qc, ensval, kld, lev, val2) &
        BIND(C, name='letkf_h08_rows_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t, letkf_h08_params
      TYPE(c_ptr), VALUE :: ctx, set, idx, slot_of_prof, lev3, sfc, pflag, btall, btclr, trans, rig, rjg, qc, ensval, lev, val2
      TYPE(letkf_h08_params), INTENT(IN) :: p
      INTEGER(c_int64_t), VALUE :: row0, nrows, nsel, kld
      INTEGER(c_int32_t), VALUE :: h08_set, nmem, m0, qc_replace
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

END MODULE letkf_h08_amd
