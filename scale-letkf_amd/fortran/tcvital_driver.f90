!===============================================================================
! tcvital_driver.f90 -- the TC vitals called from Fortran (INTEGRATION.md): letkf_tcvital_rows_dev on the decoded columns of a
! file, letkf_tcvital_search_dev for the members of one subdomain, letkf_tcvital_fill_dev with that subdomain alone (nproc = 1).
! Reads a case written by tests/test_fortran_tcvital.py, uploads it, runs the three entries, downloads and writes the results.
!   file layout (little endian, stream):
!     int32 nlon, nlat, ihalo, jhalo, nmem, m0, kld, n, i_off, j_off, qc_replace
!     real64 dx, dy, cxg1, cyg1, tc_search_dis, slot_lb, slot_ub, ritc, rjtc
!     real64 v2d(nlonh, nlath, 7, nmem)
!     int32 elm(n) ; real64 dif(n)
!     int32 qc(n) ; real64 ensval(kld, n)       (obsda row r is file row r)
!   output: int64 rows(3) ; int32 valid ; real64 cand(3, nmem) ; int32 qc(n) ; real64 ensval(kld, n)
!===============================================================================
PROGRAM tcvital_driver
  USE letkf_tcvital_amd
  IMPLICIT NONE
  INTEGER(c_int32_t) :: nlon, nlat, ihalo, jhalo, nmem, m0, kld, n, i_off, j_off, qc_replace, valid
  REAL(c_double) :: dx, dy, cxg1, cyg1, dis, slot_lb, slot_ub
  REAL(c_double), TARGET :: centre(2)
  INTEGER(c_int64_t) :: rows(3), orows(3), nlonh, nlath
  INTEGER(c_int32_t), ALLOCATABLE, TARGET :: elm(:), qc(:)
  REAL(c_double), ALLOCATABLE, TARGET :: v2d(:, :, :, :), dif(:), ensval(:, :), cand(:, :)
  INTEGER :: u, ios
  INTEGER(c_int) :: rc
  TYPE(c_ptr) :: ctx, d_v2d, d_elm, d_dif, d_qc, d_ens, d_cand, d_centre
  TYPE(letkf_tcvital_params) :: p
  TYPE(letkf_obsope_fields) :: f
  CHARACTER(len=512) :: fin, fout

  CALL get_command_argument(1, fin)
  CALL get_command_argument(2, fout)
  OPEN (newunit=u, file=trim(fin), access='stream', form='unformatted', status='old', iostat=ios)
  IF (ios /= 0) STOP 3
  READ (u) nlon, nlat, ihalo, jhalo, nmem, m0, kld, n, i_off, j_off, qc_replace
  READ (u) dx, dy, cxg1, cyg1, dis, slot_lb, slot_ub, centre
  nlonh = nlon + 2*ihalo
  nlath = nlat + 2*jhalo
  ALLOCATE (v2d(nlonh, nlath, 7, nmem), elm(n), dif(n), qc(n), ensval(kld, n), cand(3, nmem))
  READ (u) v2d
  READ (u) elm, dif
  READ (u) qc, ensval
  CLOSE (u)

  CALL chk(letkf_ctx_create(0_c_int, ctx), 'ctx_create')
  d_v2d = up(c_loc(v2d), 8_c_size_t*nlonh*nlath*7*nmem)
  d_elm = up(c_loc(elm), 4_c_size_t*n)
  d_dif = up(c_loc(dif), 8_c_size_t*n)
  d_qc = up(c_loc(qc), 4_c_size_t*n)
  d_ens = up(c_loc(ensval), 8_c_size_t*kld*n)
  d_centre = up(c_loc(centre), 16_c_size_t)
  cand = -1.0d0
  d_cand = up(c_loc(cand), 8_c_size_t*3*nmem)

  ! which rows, and whether they are a report of this slot
  CALL chk(letkf_tcvital_rows_dev(ctx, INT(n, c_int64_t), d_elm, d_dif, slot_lb, slot_ub, rows, valid), 'tcvital_rows')

  ! this subdomain's candidates: only v2d, its strides, the sizes and the halos of the fields are read
  p%dx = dx; p%dy = dy; p%cxg1 = cxg1; p%cyg1 = cyg1; p%i_off = i_off; p%j_off = j_off; p%tc_search_dis = dis
  f%nlev = 1; f%nlon = nlon; f%nlat = nlat; f%khalo = 0; f%ihalo = ihalo; f%jhalo = jhalo
  f%nv3dd = 13; f%nv2dd = 7; f%nmem = nmem; f%m0 = m0
  f%v3d = c_null_ptr; f%s3k = 1; f%s3i = 1; f%s3j = 1; f%s3v = 1; f%s3m = 1
  f%v2d = d_v2d; f%s2i = 1; f%s2j = nlonh; f%s2v = nlonh*nlath; f%s2m = 7*nlonh*nlath
  CALL chk(letkf_tcvital_search_dev(ctx, p, f, d_centre, c_ptr_plus(d_centre, 8_c_size_t), d_cand), 'tcvital_search')

  ! one subdomain: cand is cand_all; the obsda rows are the file rows, 0-based
  IF (valid == 1) THEN
    orows = rows - 1
    CALL chk(letkf_tcvital_fill_dev(ctx, 1_c_int32_t, nmem, m0, d_cand, orows, qc_replace, d_qc, d_ens, INT(kld, c_int64_t)), &
             'tcvital_fill')
  END IF
  CALL chk(letkf_ctx_synchronize(ctx), 'synchronize')

  CALL chk(hipMemcpy(c_loc(cand), d_cand, 8_c_size_t*3*nmem, hipMemcpyDeviceToHost), 'download cand')
  CALL chk(hipMemcpy(c_loc(qc), d_qc, 4_c_size_t*n, hipMemcpyDeviceToHost), 'download qc')
  CALL chk(hipMemcpy(c_loc(ensval), d_ens, 8_c_size_t*kld*n, hipMemcpyDeviceToHost), 'download ensval')
  OPEN (newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
  WRITE (u) rows, valid, cand, qc, ensval
  CLOSE (u)
  rc = letkf_ctx_destroy(ctx)

CONTAINS

  FUNCTION c_ptr_plus(base, nbytes) RESULT(q)
    TYPE(c_ptr), INTENT(IN) :: base
    INTEGER(c_size_t), INTENT(IN) :: nbytes
    TYPE(c_ptr) :: q
    q = TRANSFER(TRANSFER(base, 0_c_intptr_t) + INT(nbytes, c_intptr_t), q)
  END FUNCTION c_ptr_plus

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

END PROGRAM tcvital_driver
