!===============================================================================
! letkf_tcvital_amd.f90 -- Fortran side of include/letkf_amd_tcvital.h: TC vitals on the device.  The BIND(C) mirror of
! letkf_tcvital_params (fields in C order) and the interfaces of the three entries of libletkf_amd_tcvital.so; letkf_obsope_fields
! is the operator's module's.  The order of calls for a host (INTEGRATION.md): decode, phys2ij, the first scan, the operator for
! all members, then
!   letkf_tcvital_rows_dev    stands where obsope_cal notes obs_idx_TCX / TCY / TCP (scale/obs/obsope_tools.f90:154-204) and tests
!                             them (:651-656); rows and valid are HOST variables
!   letkf_tcvital_search_dev  stands where search_tc_subdom is called (:671); ritc / rjtc are DEVICE pointers to the TCX row's
!                             grid coordinates as phys2ij left them
!   (the host's MPI_ALLGATHER of cand over the subdomains, where :675 has its MPI_ALLREDUCE)
!   letkf_tcvital_fill_dev    stands where bTC_proc is picked and the three obsda rows are written (:678-703); rows are 0-based
!                             obsda rows on this rank, negative where the row is another rank's
! and set_letkf_obs.
!===============================================================================
MODULE letkf_tcvital_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_obsope_amd
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_TCVITAL_VERSION = 1
  INTEGER(c_int32_t), PARAMETER :: LETKF_TCVITAL_QC_BAD = 50

  TYPE, BIND(C) :: letkf_tcvital_params
    REAL(c_double)     :: dx, dy, cxg1, cyg1
    INTEGER(c_int32_t) :: i_off, j_off                               ! rank_i * nlon, rank_j * nlat
    REAL(c_double)     :: tc_search_dis
  END TYPE letkf_tcvital_params

  INTERFACE
    FUNCTION letkf_tcvital_rows_dev(ctx, n, elm, dif, slot_lb, slot_ub, rows, valid) &
        BIND(C, name='letkf_tcvital_rows_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t, c_double
      TYPE(c_ptr), VALUE :: ctx, elm, dif
      INTEGER(c_int64_t), VALUE :: n
      REAL(c_double), VALUE :: slot_lb, slot_ub
      INTEGER(c_int64_t), INTENT(OUT) :: rows(3)
      INTEGER(c_int32_t), INTENT(OUT) :: valid
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_tcvital_search_dev(ctx, p, f, ritc, rjtc, cand) BIND(C, name='letkf_tcvital_search_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_tcvital_params, letkf_obsope_fields
      TYPE(c_ptr), VALUE :: ctx, ritc, rjtc, cand
      TYPE(letkf_tcvital_params), INTENT(IN) :: p
      TYPE(letkf_obsope_fields), INTENT(IN) :: f
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_tcvital_fill_dev(ctx, nproc, nmem, m0, cand_all, rows, qc_replace, qc, ensval, kld) &
        BIND(C, name='letkf_tcvital_fill_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t
      TYPE(c_ptr), VALUE :: ctx, cand_all, qc, ensval
      INTEGER(c_int32_t), VALUE :: nproc, nmem, m0, qc_replace
      INTEGER(c_int64_t), INTENT(IN) :: rows(3)
      INTEGER(c_int64_t), VALUE :: kld
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

END MODULE letkf_tcvital_amd
