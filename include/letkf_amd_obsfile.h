/* letkf_amd_obsfile.h -- the observation, obsda and departure file records on the device: decode, assemble, encode.  The
 * reference's two programs (obsope, letkf) meet in files of Fortran sequential unformatted float32 records; between those files
 * and the device arrays of the other companions stood a per-row host loop (strip the markers, scale in single precision, NINT,
 * widen, interleave MEMBER files into the member-fastest ensval table).  This header puts that loop on the device.
 *
 * Companion of letkf_amd.h; it includes letkf_amd_mapproj.h for the letkf_mapproj struct (the TC position rows are projected).
 * The entries are exported by a library of their own, libletkf_amd_obsfile.so, which links against libletkf_amd.so for the
 * context, its stream, its scratch buffer, its scan plumbing and the error text.  DESIGN.md section 20.
 *
 * NO ENTRY TOUCHES A FILE.  A file image is the file's bytes in device memory, 4-byte aligned; the host keeps open / read /
 * write of bytes and nothing else.
 *
 * FORMATS.  A record is an int32 marker equal to 4 * nrec, then nrec float32 values wk(1:nrec), then the same marker again: what
 * gfortran, amdflang, ifort and the K compiler write for short records.  Every entry takes big_endian: non-zero means that
 * markers and values are byte-swapped (the -convert big_endian lines of scale/arch/configure.user.*).
 *   format                        nrec                       head                        scale/common/common_obs_scale.f90
 *   1 LETKF_OBSFILE_CONV          8                          none                        read_obs / write_obs :2148-2273
 *   2 LETKF_OBSFILE_RADAR         7, 8 with RADAR_OBS_4D     3 records of one float:     get_nobs_radar / read_obs_radar /
 *                                                            radar lon, lat, z           write_obs_radar :2411-2594
 *   3 LETKF_OBSFILE_OBSDA         4, 6 under -DH08           none                        read_obs_da / write_obs_da :2275-2352
 *   4 LETKF_OBSFILE_DEP           11                         none                        write_obs_dep :2354-2409
 * The H08 observation format (read_obs_H08) is handled by letkf_amd_h08.h, not here.
 * wk = elm, lon, lat, lev, dat, err, typ, dif (conventional, radar); set, idx, value, qc [, lev, val2] (obsda); the eight of the
 * file row, then qc, omb, oma (departure).
 *
 * SINGLE PRECISION.  The SELECT CASE(NINT(wk(1))) of read_obs (:2162-2198) is applied IN FLOAT32, BEFORE THE WIDENING, as the
 * reference applies it to wk: wk * 100.0f (hPa to Pa) and wk * 0.01f (percent), err = float32(OBSERR_TCP / TCX / TCY) for the TC
 * ids, and for the TC position ids 99991 / 99992 dat = float32(x) or float32(y) of the Lambert forward projection at
 * lon * pi / 180, lat * pi / 180 with the reference's 10-digit pi.  The encoders narrow each double to float32 (round to nearest
 * even) and then apply the SELECT CASE of write_obs (:2245-2266) or write_obs_dep (:2382-2403) in float32.  float32 denormals are
 * kept (1e-37f * 0.01f is not flushed).  NINT of a float32 rounds half away from zero.
 * NEW, not in the reference:  NINT(NaN) = 0 and NINT saturates at the ends of int32;  with proj NULL a TC position row's dat is
 * NaN;  a record whose markers are wrong is decoded all the same and counted (nbad);  the DEBUG check of letkf_obs.f90:219-226
 * is a count (ninconsistent) instead of a stop.
 *
 * letkf_obsfile_count (host only): get_nobs / get_nobs_radar (:2124, :2479-2481) -- the rows of a file of nbytes, or
 *   LETKF_E_INVALID when nbytes is not a head plus a whole number of records.  letkf_obsfile_bytes is the inverse.
 * letkf_obs_decode_dev: a conventional or radar image to the columns of o (each may be NULL).  Radar rows get typ = 22, and
 *   dif = 0 when nrec = 7 (:2526-2538); meta (HOST [3] or NULL) takes the three head values as doubles and costs the read-back
 *   of 36 bytes.  nbad (HOST or NULL): the number of records whose two markers are not 4 * nrec; NULL means no check, no
 *   read-back and no synchronisation.  p->proj_given = 0: proj is not read.
 * letkf_obs_encode_dev: the inverse, write_obs / write_obs_radar.  Radar: the three head records from meta (HOST [3], required).
 *   p->missing = 0 (write_obs_all(..., missing=.false.), obsope_tools.f90:1055): a row is written only where
 *   abs(dat - undef) > tiny(1.0f) in double, undef = -9.99d33; the survivors keep their order (a stable compaction: block
 *   counts, the main library's scan, block-local ranks; no shared counter decides a position) and their number comes back in
 *   *nwritten (HOST, required then) -- the entry's one read-back.  p->missing != 0: every row, no read-back; *nwritten = nrows
 *   where given.  The image must hold letkf_obsfile_bytes(nrows) bytes in both cases.
 * letkf_obsda_assemble_dev: p->nmem obsda images of p->nobs records each (images: HOST array of device pointers) into the
 *   member-fastest table, the member loop of letkf_obs.f90:180-237 with obs_da_value_partial_reduce_iter
 *   (common_mpi_scale.f90:1834-1874):  ensval[n * kld + col[m]] = double(wk(3)) (col: HOST [nmem], distinct, 0 <= col < kld --
 *   the mean or deterministic file lands where the caller says, as obsda%ensval(mmdetobs,:) does in :1932-1945; other columns are
 *   untouched);  set[n] / idx[n] = NINT(wk(1)) / NINT(wk(2)) of image 0;  qc[n] INOUT = max(qc[n], NINT(wk(4)) of every image);
 *   under nrec = 6, lev[n] / val2[n] INOUT += the wk(5) / wk(6) of the images with is_member[m] != 0 (HOST [nmem]; NULL: all),
 *   summed sequentially in image order from the caller's value by one writer, then divided by double(p->member) where p->finish
 *   (:1867-1870, :1959-1960).  ninconsistent (HOST or NULL): rows whose set or idx differs between image 0 and any other.
 *   nbad as above, over all images.  The table of images leaves pageable host memory: the entry synchronises the stream once, with
 *   or without the counts.  One kernel: a block takes LETKF_OBSFILE_TILE_ROWS rows and walks
 *   the images LETKF_OBSFILE_TILE_MEMBERS at a time; each image byte is read once, with coalesced loads along the image; the tile
 *   is transposed through padded LDS; ensval is written as member-fastest row segments; no atomics, one writer per value, results
 *   bitwise equal from call to call.  nmem 1 .. 65536, kld < 2^20, nobs < 2^31.
 * letkf_obsda_encode_dev: write_obs_da for column col of ensval, or val when col < 0 (im == 0): float32(set), float32(idx) --
 *   rounded above 2^24 as the reference's "will overflow" comment says, not refused --, float32(value), float32(qc), and lev,
 *   val2 under nrec = 6.
 * letkf_obsdep_encode_dev: write_obs_dep for nobs rows of set / idx (1-based file and row), qc, omb, oma, gathering the eight
 *   columns of the file rows.  A set / idx outside the files is found by a device check whose count is read back with the
 *   entry's only synchronisation, before anything is written.
 *
 * REFUSED with LETKF_E_INVALID and an error text that names the argument, nothing written: NULL required pointers; an image
 * pointer not 4-byte aligned; a format the entry does not take, or nrec not one the format allows; negative counts (and nrows or
 * nobs of 2^31 or more); nmem outside 1 .. 65536; kld < 1 or >= 2^20; col out of range or repeated; member < 1 with finish;
 * outputs overlapping inputs or each other; proj_given with a proj of a type other than 1; a set / idx outside the files.  Zero
 * rows is no error and launches nothing.
 */
#ifndef LETKF_AMD_OBSFILE_H
#define LETKF_AMD_OBSFILE_H

#include "letkf_amd_mapproj.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LETKF_AMD_OBSFILE_VERSION 1
#define LETKF_OBSFILE_CONV 1
#define LETKF_OBSFILE_RADAR 2
#define LETKF_OBSFILE_OBSDA 3
#define LETKF_OBSFILE_DEP 4
#define LETKF_OBSFILE_TILE_ROWS 64       /* rows of the assemble kernel's tile */
#define LETKF_OBSFILE_TILE_MEMBERS 16    /* images of the assemble kernel's tile */
#define LETKF_OBSFILE_MAX_MEMBERS 65536
#define LETKF_OBSFILE_TYP_RADAR 22       /* :2533 */

typedef struct {          /* the decoded columns of a conventional or radar file: dev [nrows] */
  int32_t *elm, *typ;
  double *lon, *lat, *lev, *dat, *err, *dif;
} letkf_obsfile_cols;

typedef struct {
  int32_t format;                                 /* LETKF_OBSFILE_CONV or LETKF_OBSFILE_RADAR */
  int32_t nrec;                                   /* 8; radar: 7 or 8 */
  int32_t big_endian;
  int32_t missing;                                /* encode: 0 = undefined rows are left out */
  int32_t proj_given, reserved0;                  /* decode: non-zero = proj is read */
  double obserr_tcp, obserr_tcx, obserr_tcy;      /* decode: OBSERR_TCP / TCX / TCY (common_nml.f90:306-308) */
} letkf_obsfile_params;

typedef struct {
  int32_t nrec;                                   /* 4, or 6 (-DH08) */
  int32_t big_endian;
  int32_t nmem;                                   /* images */
  int32_t finish;                                 /* nrec 6: non-zero = divide lev / val2 by member */
  int32_t member, reserved0;                      /* MEMBER */
  int64_t nobs, kld;
} letkf_obsda_params;

typedef struct {          /* the obsda arrays: dev [nobs], ensval dev [nobs][kld] */
  int32_t *set, *idx, *qc;
  double *ensval, *lev, *val2;                    /* lev, val2: nrec 6 only, may be NULL */
} letkf_obsda_cols;

typedef struct {          /* the observation files flattened into one row space: file f owns rows off[f] .. off[f+1]-1 */
  int32_t nfile, reserved0;
  const int64_t *off;                             /* HOST [nfile + 1] */
  const int32_t *elm, *typ;                       /* dev [off[nfile]] */
  const double *lon, *lat, *lev, *dat, *err, *dif;
} letkf_obsfile_rows;

int letkf_obsfile_count(int32_t format, int32_t nrec, int64_t nbytes, int64_t *nrows);
int letkf_obsfile_bytes(int32_t format, int32_t nrec, int64_t nrows, int64_t *nbytes);

int letkf_obs_decode_dev(letkf_ctx *ctx, const letkf_obsfile_params *p, const letkf_mapproj *proj, const uint32_t *image,
                         int64_t nrows, const letkf_obsfile_cols *o, double *meta, int64_t *nbad);
int letkf_obs_encode_dev(letkf_ctx *ctx, const letkf_obsfile_params *p, int64_t nrows, const letkf_obsfile_cols *in,
                         const double *meta, uint32_t *image, int64_t *nwritten);

int letkf_obsda_assemble_dev(letkf_ctx *ctx, const letkf_obsda_params *p, const uint32_t *const *images, const int32_t *col,
                             const int32_t *is_member, const letkf_obsda_cols *o, int64_t *ninconsistent, int64_t *nbad);
int letkf_obsda_encode_dev(letkf_ctx *ctx, int32_t nrec, int32_t big_endian, int64_t nobs, const int32_t *set,
                           const int32_t *idx, const int32_t *qc, const double *ensval, int64_t kld, int32_t col,
                           const double *val, const double *lev, const double *val2, uint32_t *image);

int letkf_obsdep_encode_dev(letkf_ctx *ctx, int32_t big_endian, int64_t nobs, const int32_t *set, const int32_t *idx,
                            const int32_t *qc, const double *omb, const double *oma, const letkf_obsfile_rows *files,
                            uint32_t *image);

#ifdef __cplusplus
}
#endif
#endif
