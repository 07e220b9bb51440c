!===============================================================================
! letkf_mapproj_amd.f90 -- Fortran side of include/letkf_amd_mapproj.h: the map projection on the device.  The BIND(C) mirrors of
! letkf_mapproj_params and letkf_mapproj (fields in C order), the interfaces of the entries of libletkf_amd_mapproj.so, and
!   mapproj_setup_amd   stands where MPRJ_setup's values are read: PARAM_MAPPROJ, GRID_CXG(1), GRID_CYG(1), DX, DY in, proj out
!   phys2ij_amd         stands where the loop over a file's rows called phys2ij (and MPRJ_rotcoef): lon, lat -> ri, rj, rotc
!   ij2phys_amd         the same the other way
!   mapproj_grid_amd    stands where the loop of common_mpi_scale.f90:193-203 filled lon2d / lat2d
! Lambert conformal conic only.  All arrays are DEVICE arrays; the calls are asynchronous on the context's stream.
!===============================================================================
MODULE letkf_mapproj_amd
  USE, INTRINSIC :: iso_c_binding
  USE letkf_amd_api
  IMPLICIT NONE
  PUBLIC

  INTEGER(c_int), PARAMETER :: LETKF_AMD_MAPPROJ_VERSION = 1
  INTEGER(c_int32_t), PARAMETER :: LETKF_MAPPROJ_LC = 1
  REAL(c_double), PARAMETER :: LETKF_MAPPROJ_RADIUS_SCALE = 6.37122d6

  TYPE, BIND(C) :: letkf_mapproj_params
    INTEGER(c_int32_t) :: type, reserved0                           ! 1 = LC
    REAL(c_double)     :: basepoint_lon, basepoint_lat              ! degrees
    REAL(c_double)     :: basepoint_x, basepoint_y                  ! m
    REAL(c_double)     :: lc_lat1, lc_lat2                          ! degrees, lc_lat1 < lc_lat2
    REAL(c_double)     :: radius
    REAL(c_double)     :: cxg1, cyg1                                ! GRID_CXG(1), GRID_CYG(1)
    REAL(c_double)     :: dx, dy
  END TYPE letkf_mapproj_params

  TYPE, BIND(C) :: letkf_mapproj
    INTEGER(c_int32_t) :: type, reserved0
    REAL(c_double)     :: hemisphere
    REAL(c_double)     :: lon0
    REAL(c_double)     :: c, fact, radius
    REAL(c_double)     :: pole_x, pole_y
    REAL(c_double)     :: cxg1, cyg1, dx, dy
  END TYPE letkf_mapproj

  INTERFACE
    FUNCTION letkf_mapproj_setup(p, proj) BIND(C, name='letkf_mapproj_setup') RESULT(rc)
      IMPORT :: c_int, letkf_mapproj_params, letkf_mapproj
      TYPE(letkf_mapproj_params), INTENT(IN) :: p
      TYPE(letkf_mapproj), INTENT(OUT) :: proj
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_phys2ij_dev(ctx, proj, n, lon, lat, ri, rj, rotc) BIND(C, name='letkf_phys2ij_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t, letkf_mapproj
      TYPE(c_ptr), VALUE :: ctx, lon, lat, ri, rj, rotc
      TYPE(letkf_mapproj), INTENT(IN) :: proj
      INTEGER(c_int64_t), VALUE :: n
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_ij2phys_dev(ctx, proj, n, ri, rj, lon, lat, rotc) BIND(C, name='letkf_ij2phys_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int64_t, letkf_mapproj
      TYPE(c_ptr), VALUE :: ctx, ri, rj, lon, lat, rotc
      TYPE(letkf_mapproj), INTENT(IN) :: proj
      INTEGER(c_int64_t), VALUE :: n
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_mapproj_grid_dev(ctx, proj, nlon, nlat, ihalo, jhalo, cx1, cy1, lon2d, lat2d, rotc2d) &
        BIND(C, name='letkf_mapproj_grid_dev') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_int32_t, c_double, letkf_mapproj
      TYPE(c_ptr), VALUE :: ctx, lon2d, lat2d, rotc2d
      TYPE(letkf_mapproj), INTENT(IN) :: proj
      INTEGER(c_int32_t), VALUE :: nlon, nlat, ihalo, jhalo
      REAL(c_double), VALUE :: cx1, cy1
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_phys2ij_host(proj, lon, lat, ri, rj, rotc) BIND(C, name='letkf_phys2ij_host') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_double, letkf_mapproj
      TYPE(letkf_mapproj), INTENT(IN) :: proj
      REAL(c_double), VALUE :: lon, lat
      REAL(c_double), INTENT(OUT) :: ri, rj
      TYPE(c_ptr), VALUE :: rotc                                     ! HOST real64 (2), or c_null_ptr
      INTEGER(c_int) :: rc
    END FUNCTION
    FUNCTION letkf_ij2phys_host(proj, ri, rj, lon, lat, rotc) BIND(C, name='letkf_ij2phys_host') RESULT(rc)
      IMPORT :: c_int, c_ptr, c_double, letkf_mapproj
      TYPE(letkf_mapproj), INTENT(IN) :: proj
      REAL(c_double), VALUE :: ri, rj
      REAL(c_double), INTENT(OUT) :: lon, lat
      TYPE(c_ptr), VALUE :: rotc
      INTEGER(c_int) :: rc
    END FUNCTION
  END INTERFACE

CONTAINS

  ! PARAM_MAPPROJ (degrees, metres; LC) and the grid's GRID_CXG(1), GRID_CYG(1), DX, DY; radius: CONST_RADIUS when absent
  SUBROUTINE mapproj_setup_amd(basepoint_lon, basepoint_lat, basepoint_x, basepoint_y, lc_lat1, lc_lat2, cxg1, cyg1, dx, dy, proj, &
                               ierr, radius)
    REAL(c_double), INTENT(IN) :: basepoint_lon, basepoint_lat, basepoint_x, basepoint_y, lc_lat1, lc_lat2, cxg1, cyg1, dx, dy
    TYPE(letkf_mapproj), INTENT(OUT) :: proj
    INTEGER, INTENT(OUT) :: ierr
    REAL(c_double), INTENT(IN), OPTIONAL :: radius
    TYPE(letkf_mapproj_params) :: p

    p%type = LETKF_MAPPROJ_LC; p%reserved0 = 0
    p%basepoint_lon = basepoint_lon; p%basepoint_lat = basepoint_lat; p%basepoint_x = basepoint_x; p%basepoint_y = basepoint_y
    p%lc_lat1 = lc_lat1; p%lc_lat2 = lc_lat2; p%cxg1 = cxg1; p%cyg1 = cyg1; p%dx = dx; p%dy = dy
    p%radius = LETKF_MAPPROJ_RADIUS_SCALE
    IF (PRESENT(radius)) p%radius = radius
    ierr = letkf_mapproj_setup(p, proj)
  END SUBROUTINE mapproj_setup_amd

  ! n rows: lon, lat (degrees) -> ri, rj and, when present, rotc (2, n)
  SUBROUTINE phys2ij_amd(ctx, proj, n, lon, lat, ri, rj, ierr, rotc)
    TYPE(c_ptr), INTENT(IN) :: ctx, lon, lat, ri, rj
    TYPE(letkf_mapproj), INTENT(IN) :: proj
    INTEGER(c_int64_t), INTENT(IN) :: n
    INTEGER, INTENT(OUT) :: ierr
    TYPE(c_ptr), INTENT(IN), OPTIONAL :: rotc
    TYPE(c_ptr) :: r

    r = c_null_ptr
    IF (PRESENT(rotc)) r = rotc
    ierr = letkf_phys2ij_dev(ctx, proj, n, lon, lat, ri, rj, r)
  END SUBROUTINE phys2ij_amd

  SUBROUTINE ij2phys_amd(ctx, proj, n, ri, rj, lon, lat, ierr, rotc)
    TYPE(c_ptr), INTENT(IN) :: ctx, ri, rj, lon, lat
    TYPE(letkf_mapproj), INTENT(IN) :: proj
    INTEGER(c_int64_t), INTENT(IN) :: n
    INTEGER, INTENT(OUT) :: ierr
    TYPE(c_ptr), INTENT(IN), OPTIONAL :: rotc
    TYPE(c_ptr) :: r

    r = c_null_ptr
    IF (PRESENT(rotc)) r = rotc
    ierr = letkf_ij2phys_dev(ctx, proj, n, ri, rj, lon, lat, r)
  END SUBROUTINE ij2phys_amd

  ! lon2d, lat2d (nlon, nlat) and rotc2d (2, nlon, nlat) of the subdomain whose GRID_CX(1) / GRID_CY(1) are cx1 / cy1; an output
  ! that is c_null_ptr is not made
  SUBROUTINE mapproj_grid_amd(ctx, proj, nlon, nlat, ihalo, jhalo, cx1, cy1, lon2d, lat2d, rotc2d, ierr)
    TYPE(c_ptr), INTENT(IN) :: ctx, lon2d, lat2d, rotc2d
    TYPE(letkf_mapproj), INTENT(IN) :: proj
    INTEGER, INTENT(IN) :: nlon, nlat, ihalo, jhalo
    REAL(c_double), INTENT(IN) :: cx1, cy1
    INTEGER, INTENT(OUT) :: ierr

    ierr = letkf_mapproj_grid_dev(ctx, proj, INT(nlon, c_int32_t), INT(nlat, c_int32_t), INT(ihalo, c_int32_t), &
                                  INT(jhalo, c_int32_t), cx1, cy1, lon2d, lat2d, rotc2d)
  END SUBROUTINE mapproj_grid_amd

END MODULE letkf_mapproj_amd
