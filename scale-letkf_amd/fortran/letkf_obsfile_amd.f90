!===============================================================================
! letkf_obsfile_amd.f90 -- Fortran side of include/letkf_amd_obsfile.h: the records of the observation, obsda and departure files
! on the device.  The BIND(C) mirrors of the header's structs (fields in C order), the interfaces of the entries of
! libletkf_amd_obsfile.so, and
!   obsfile_count_amd     stands where get_nobs / get_nobs_radar divided the file's size
!   obs_decode_amd        stands where read_obs / read_obs_radar looped over READ(iunit) wk
!   obs_encode_amd        stands where write_obs / write_obs_radar looped over WRITE(iunit) wk
!   obsda_assemble_amd    stands where the member loop of set_letkf_obs called read_obs_da and obs_da_value_partial_reduce_iter
!   obsda_encode_amd      stands where write_obs_da looped
!   obsdep_encode_amd     stands where write_obs_dep looped
! The host keeps OPEN / READ / WRITE of the file's bytes (ACCESS='stream'); an image is those bytes in DEVICE memory.
!===============================================================================
MODULE letkf_obsfile_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_mapproj_amd
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_OBSFILE_VERSION = 1
  INTEGER(c_int32_t), PARAMETER :: LETKF_OBSFILE_CONV = 1, LETKF_OBSFILE_RADAR = 2, LETKF_OBSFILE_OBSDA = 3, LETKF_OBSFILE_DEP = 4
  INTEGER(c_int32_t), PARAMETER :: LETKF_OBSFILE_TILE_ROWS = 64, LETKF_OBSFILE_TILE_MEMBERS = 16

  TYPE, BIND(C) :: letkf_obsfile_cols
    TYPE(c_ptr) :: elm, typ                                          ! dev int32 (nrows)
    TYPE(c_ptr) :: lon, lat, lev, dat, err, dif                      ! dev real64 (nrows)
  END TYPE letkf_obsfile_cols

  TYPE, BIND(C) :: letkf_obsfile_params
    INTEGER(c_int32_t) :: format                                     ! LETKF_OBSFILE_CONV or LETKF_OBSFILE_RADAR
    INTEGER(c_int32_t) :: nrec                                       ! 8; radar: 7 or 8
    INTEGER(c_int32_t) :: big_endian
    INTEGER(c_int32_t) :: missing                                    ! encode: 0 = undefined rows are left out
    INTEGER(c_int32_t) :: proj_given, reserved0
    REAL(c_double)     :: obserr_tcp, obserr_tcx, obserr_tcy
  END TYPE letkf_obsfile_params

  TYPE, BIND(C) :: letkf_obsda_params
    INTEGER(c_int32_t) :: nrec                                       ! 4, or 6 (-DH08)
    INTEGER(c_int32_t) :: big_endian
    INTEGER(c_int32_t) :: nmem
    INTEGER(c_int32_t) :: finish
    INTEGER(c_int32_t) :: member, reserved0
    INTEGER(c_int64_t) :: nobs, kld
  END TYPE letkf_obsda_params

  TYPE, BIND(C) :: letkf_obsda_cols
    TYPE(c_ptr) :: set, idx, qc                                      ! dev int32 (nobs)
    TYPE(c_ptr) :: ensval, lev, val2                                 ! dev real64 (kld, nobs), (nobs), (nobs)
  END TYPE letkf_obsda_cols

  TYPE, BIND(C) :: letkf_obsfile_rows
    INTEGER(c_int32_t) :: nfile, reserved0
    TYPE(c_ptr) :: off                                               ! HOST int64 (nfile + 1)
    TYPE(c_ptr) :: elm, typ
    TYPE(c_ptr) :: lon, lat, lev, dat, err, dif
  END TYPE letkf_obsfile_rows

  INTERFACE
    FUNCTION letkf_obsfile_count(format, nrec, nbytes, nrows) BIND(C, name='letkf_obsfile_count') RESULT(rc)
      IMPORT :: c_int, c_int32_t, c_int64_t
      INTEGER(c_int32_t), VALUE :: format, nrec
      INTEGER(c_int64_t), VALUE :: nbytes
      INTEGER(c_int64_t), INTENT(OUT) :: nrows
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obsfile_bytes(format, nrec, nrows, nbytes) BIND(C, name='letkf_obsfile_bytes') RESULT(rc)
      IMPORT :: c_int, c_int32_t, c_int64_t
      INTEGER(c_int32_t), VALUE :: format, nrec
      INTEGER(c_int64_t), VALUE :: nrows
      INTEGER(c_int64_t), INTENT(OUT) :: nbytes
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obs_decode_dev(ctx, p, proj, image, nrows, o, meta, nbad) BIND(C, name='letkf_obs_decode_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t, letkf_obsfile_params, letkf_obsfile_cols
      TYPE(c_ptr), VALUE :: ctx, proj, image, meta, nbad             ! proj: c_loc of a letkf_mapproj or c_null_ptr; meta, nbad: HOST
      TYPE(letkf_obsfile_params), INTENT(IN) :: p
      INTEGER(c_int64_t), VALUE :: nrows
      TYPE(letkf_obsfile_cols), INTENT(IN) :: o
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obs_encode_dev(ctx, p, nrows, cols, meta, image, nwritten) BIND(C, name='letkf_obs_encode_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t, letkf_obsfile_params, letkf_obsfile_cols
      TYPE(c_ptr), VALUE :: ctx, meta, image, nwritten
      TYPE(letkf_obsfile_params), INTENT(IN) :: p
      INTEGER(c_int64_t), VALUE :: nrows
      TYPE(letkf_obsfile_cols), INTENT(IN) :: cols
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obsda_assemble_dev(ctx, p, images, col, is_member, o, ninconsistent, nbad) &
        BIND(C, name='letkf_obsda_assemble_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, letkf_obsda_params, letkf_obsda_cols
      TYPE(c_ptr), VALUE :: ctx, images, col, is_member, ninconsistent, nbad     ! HOST arrays; images: c_ptr (nmem) of device images
      TYPE(letkf_obsda_params), INTENT(IN) :: p
      TYPE(letkf_obsda_cols), INTENT(IN) :: o
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obsda_encode_dev(ctx, nrec, big_endian, nobs, set, idx, qc, ensval, kld, col, val, lev, val2, image) &
        BIND(C, name='letkf_obsda_encode_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t
      TYPE(c_ptr), VALUE :: ctx, set, idx, qc, ensval, val, lev, val2, image
      INTEGER(c_int32_t), VALUE :: nrec, big_endian, col
      INTEGER(c_int64_t), VALUE :: nobs, kld
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_obsdep_encode_dev(ctx, big_endian, nobs, set, idx, qc, omb, oma, files, image) &
        BIND(C, name='letkf_obsdep_encode_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_int64_t, letkf_obsfile_rows
      TYPE(c_ptr), VALUE :: ctx, set, idx, qc, omb, oma, image
      INTEGER(c_int32_t), VALUE :: big_endian
      INTEGER(c_int64_t), VALUE :: nobs
      TYPE(letkf_obsfile_rows), INTENT(IN) :: files
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! the rows of a file of nbytes: format 1 conventional, 2 radar, 3 obsda, 4 departure; ierr /= 0 where it is no whole number
  SUBROUTINE obsfile_count_amd(format, nrec, nbytes, nrows, ierr)
    INTEGER, INTENT(IN) :: format, nrec
    INTEGER(c_int64_t), INTENT(IN) :: nbytes
    INTEGER(c_int64_t), INTENT(OUT) :: nrows
    INTEGER, INTENT(OUT) :: ierr
    ierr = letkf_obsfile_count(INT(format, c_int32_t), INT(nrec, c_int32_t), nbytes, nrows)
  END SUBROUTINE obsfile_count_amd

  ! image (dev) -> the columns of o; meta (radar lon, lat, z) and nbad where present; proj for the TC position rows
  SUBROUTINE obs_decode_amd(ctx, p, image, nrows, o, ierr, proj, meta, nbad)
    TYPE(c_ptr), INTENT(IN) :: ctx, image
    TYPE(letkf_obsfile_params), INTENT(IN) :: p
    INTEGER(c_int64_t), INTENT(IN) :: nrows
    TYPE(letkf_obsfile_cols), INTENT(IN) :: o
    INTEGER, INTENT(OUT) :: ierr
    TYPE(letkf_mapproj), INTENT(IN), TARGET, OPTIONAL :: proj
    REAL(c_double), INTENT(OUT), TARGET, OPTIONAL :: meta(3)
    INTEGER(c_int64_t), INTENT(OUT), TARGET, OPTIONAL :: nbad
    TYPE(letkf_obsfile_params) :: q
    TYPE(c_ptr) :: pp, pm, pb

    q = p; pp = c_null_ptr; pm = c_null_ptr; pb = c_null_ptr
    q%proj_given = 0
    IF (PRESENT(proj)) THEN
      pp = c_loc(proj); q%proj_given = 1
    END IF
    IF (PRESENT(meta)) pm = c_loc(meta)
    IF (PRESENT(nbad)) pb = c_loc(nbad)
    ierr = letkf_obs_decode_dev(ctx, q, pp, image, nrows, o, pm, pb)
  END SUBROUTINE obs_decode_amd

  ! the columns -> image (dev, sized for nrows rows); nwritten: the rows written (p%missing = 0 leaves the undefined ones out)
  SUBROUTINE obs_encode_amd(ctx, p, nrows, cols, image, nwritten, ierr, meta)
    TYPE(c_ptr), INTENT(IN) :: ctx, image
    TYPE(letkf_obsfile_params), INTENT(IN) :: p
    INTEGER(c_int64_t), INTENT(IN) :: nrows
    TYPE(letkf_obsfile_cols), INTENT(IN) :: cols
    INTEGER(c_int64_t), INTENT(OUT), TARGET :: nwritten
    INTEGER, INTENT(OUT) :: ierr
    REAL(c_double), INTENT(IN), TARGET, OPTIONAL :: meta(3)
    TYPE(c_ptr) :: pm

    pm = c_null_ptr
    IF (PRESENT(meta)) pm = c_loc(meta)
    ierr = letkf_obs_encode_dev(ctx, p, nrows, cols, pm, image, c_loc(nwritten))
  END SUBROUTINE obs_encode_amd

  ! images(m) (dev, nobs records each) -> obsda%ensval(col(m) + 1, :), set, idx, qc = max(qc, ..); col is 0-based
  SUBROUTINE obsda_assemble_amd(ctx, p, images, col, o, ierr, is_member, ninconsistent, nbad)
    TYPE(c_ptr), INTENT(IN) :: ctx
    TYPE(letkf_obsda_params), INTENT(IN) :: p
    TYPE(c_ptr), INTENT(IN), TARGET :: images(p%nmem)
    INTEGER(c_int32_t), INTENT(IN), TARGET :: col(p%nmem)
    TYPE(letkf_obsda_cols), INTENT(IN) :: o
    INTEGER, INTENT(OUT) :: ierr
    INTEGER(c_int32_t), INTENT(IN), TARGET, OPTIONAL :: is_member(p%nmem)
    INTEGER(c_int64_t), INTENT(OUT), TARGET, OPTIONAL :: ninconsistent, nbad
    TYPE(c_ptr) :: pf, pi, pb

    pf = c_null_ptr; pi = c_null_ptr; pb = c_null_ptr
    IF (PRESENT(is_member)) pf = c_loc(is_member)
    IF (PRESENT(ninconsistent)) pi = c_loc(ninconsistent)
    IF (PRESENT(nbad)) pb = c_loc(nbad)
    ierr = letkf_obsda_assemble_dev(ctx, p, c_loc(images), c_loc(col), pf, o, pi, pb)
  END SUBROUTINE obsda_assemble_amd

  ! write_obs_da's image of column col (0-based) of ensval, or of val when col < 0; lev / val2: c_null_ptr unless nrec = 6
  SUBROUTINE obsda_encode_amd(ctx, nrec, nobs, set, idx, qc, ensval, kld, col, val, lev, val2, image, ierr, big_endian)
    TYPE(c_ptr), INTENT(IN) :: ctx, set, idx, qc, ensval, val, lev, val2, image
    INTEGER, INTENT(IN) :: nrec, col
    INTEGER(c_int64_t), INTENT(IN) :: nobs, kld
    INTEGER, INTENT(OUT) :: ierr
    LOGICAL, INTENT(IN), OPTIONAL :: big_endian
    INTEGER(c_int32_t) :: be

    be = 0
    IF (PRESENT(big_endian)) be = MERGE(1, 0, big_endian)
    ierr = letkf_obsda_encode_dev(ctx, INT(nrec, c_int32_t), be, nobs, set, idx, qc, ensval, kld, INT(col, c_int32_t), val, lev, val2, image)
  END SUBROUTINE obsda_encode_amd

  ! write_obs_dep's image of nobs rows
  SUBROUTINE obsdep_encode_amd(ctx, nobs, set, idx, qc, omb, oma, files, image, ierr, big_endian)
    TYPE(c_ptr), INTENT(IN) :: ctx, set, idx, qc, omb, oma, image
    INTEGER(c_int64_t), INTENT(IN) :: nobs
    TYPE(letkf_obsfile_rows), INTENT(IN) :: files
    INTEGER, INTENT(OUT) :: ierr
    LOGICAL, INTENT(IN), OPTIONAL :: big_endian
    INTEGER(c_int32_t) :: be

    be = 0
    IF (PRESENT(big_endian)) be = MERGE(1, 0, big_endian)
    ierr = letkf_obsdep_encode_dev(ctx, be, nobs, set, idx, qc, omb, oma, files, image)
  END SUBROUTINE obsdep_encode_amd

END MODULE letkf_obsfile_amd
