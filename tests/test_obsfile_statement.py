"""The numpy statement of the record formats (tests/_obsfile.py) against Fortran itself, without a device: a small program of
our own, compiled with amdflang, writes one file per format with sequential unformatted WRITE and its bytes must be the
statement's encoder output for the same values -- the framing and the marker width are the compiler's, not ours; a second program
reads the statement's files back with sequential READ.  Beside them the single-precision points of the formats, pinned by values
computed by hand."""
import os
import subprocess

import numpy as np
import pytest

import _obsfile as O

FC = "/opt/rocm/bin/amdflang"
HAVE_FC = os.path.exists(FC)
F32 = np.float32
NROW = 5
FORMATS = (("conv", 8, False), ("radar", 7, True), ("radar4d", 8, True), ("obsda", 4, False), ("obsda_h08", 6, False), ("dep", 11, False))

WRITER = """
PROGRAM obsfile_writer
  IMPLICIT NONE
  CALL one('conv.dat', 8, .FALSE.)
  CALL one('radar.dat', 7, .TRUE.)
  CALL one('radar4d.dat', 8, .TRUE.)
  CALL one('obsda.dat', 4, .FALSE.)
  CALL one('obsda_h08.dat', 6, .FALSE.)
  CALL one('dep.dat', 11, .FALSE.)
CONTAINS
  SUBROUTINE one(name, nrec, head)
    CHARACTER(*), INTENT(IN) :: name
    INTEGER, INTENT(IN) :: nrec
    LOGICAL, INTENT(IN) :: head
    REAL(4) :: wk(nrec)
    INTEGER :: n, k
    OPEN (92, FILE=name, FORM='unformatted', ACCESS='sequential', STATUS='replace')
    IF (head) THEN
      WRITE (92) REAL(135.5d0, 4)
      WRITE (92) REAL(34.75d0, 4)
      WRITE (92) REAL(88.0d0, 4)
    END IF
    DO n = 1, 5
      DO k = 1, nrec
        wk(k) = REAL(n*16 + k, 4) * 0.25 - 3.0
      END DO
      WRITE (92) wk
    END DO
    CLOSE (92)
  END SUBROUTINE one
END PROGRAM obsfile_writer
"""

READER = """
PROGRAM obsfile_reader
  IMPLICIT NONE
  CALL one('conv.dat', 8, .FALSE.)
  CALL one('radar.dat', 7, .TRUE.)
  CALL one('radar4d.dat', 8, .TRUE.)
  CALL one('obsda.dat', 4, .FALSE.)
  CALL one('obsda_h08.dat', 6, .FALSE.)
  CALL one('dep.dat', 11, .FALSE.)
CONTAINS
  SUBROUTINE one(name, nrec, head)
    CHARACTER(*), INTENT(IN) :: name
    INTEGER, INTENT(IN) :: nrec
    LOGICAL, INTENT(IN) :: head
    REAL(4) :: wk(nrec), tmp
    INTEGER :: n, k, ios
    OPEN (91, FILE=name, FORM='unformatted', ACCESS='sequential', STATUS='old')
    IF (head) THEN
      DO k = 1, 3
        READ (91) tmp
        WRITE (6, '(A,1X,A,1X,I0)') 'head', name, TRANSFER(tmp, 0)
      END DO
    END IF
    DO n = 1, 5
      READ (91) wk
      WRITE (6, '(A,1X,A,20(1X,I0))') 'row', name, (TRANSFER(wk(k), 0), k = 1, nrec)
    END DO
    READ (91, IOSTAT=ios) wk
    WRITE (6, '(A,1X,A,1X,L1)') 'end', name, ios /= 0
    CLOSE (91)
  END SUBROUTINE one
END PROGRAM obsfile_reader
"""


def values(nrec):
    """the writer's wk, row by row: exact in float32"""
    return np.array([[F32(n * 16 + k) * F32(0.25) - F32(3.0) for k in range(1, nrec + 1)] for n in range(1, NROW + 1)], dtype=F32)


def build(tmp_path, name, source):
    (tmp_path / (name + ".f90")).write_text(source)
    subprocess.check_call([FC, "-O2", str(tmp_path / (name + ".f90")), "-o", str(tmp_path / name)], cwd=tmp_path)
    return str(tmp_path / name)


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortrans_sequential_write_gives_the_statements_bytes(tmp_path):
    subprocess.check_call([build(tmp_path, "obsfile_writer", WRITER)], cwd=tmp_path)
    for name, nrec, head in FORMATS:
        got = (tmp_path / (name + ".dat")).read_bytes()
        want = O.frame(values(nrec), head=(135.5, 34.75, 88.0) if head else None)
        assert got == want, name
        assert len(got) == 4 * (9 * head + NROW * (nrec + 2))
        rec, markers, meta = O.unframe(got, nrec, head=head)
        assert (markers == 4 * nrec).all() and O.same_bits(rec, values(nrec)), name
        assert meta is None or list(meta) == [135.5, 34.75, 88.0]
    assert O.count(O.CONV, 8, 40 * NROW) == NROW and O.count(O.RADAR, 7, 36 + 36 * NROW) == NROW and O.count(O.CONV, 8, 41) is None


@pytest.mark.skipif(not HAVE_FC, reason="amdflang not present")
def test_fortrans_sequential_read_takes_the_statements_files(tmp_path):
    rng = np.random.default_rng(4)
    recs = {}
    for name, nrec, head in FORMATS:
        recs[name] = rng.normal(0.0, 100.0, (NROW, nrec)).astype(F32)
        (tmp_path / (name + ".dat")).write_bytes(O.frame(recs[name], head=(135.523, 34.823, 120.5) if head else None))
    out = subprocess.check_output([build(tmp_path, "obsfile_reader", READER)], cwd=tmp_path, text=True)
    lines = [l.split() for l in out.splitlines() if l.strip()]
    for name, nrec, head in FORMATS:
        rows = [[int(v) for v in l[2:]] for l in lines if l[0] == "row" and l[1] == name + ".dat"]
        assert np.array_equal(np.array(rows, dtype=np.int32), recs[name].view(np.int32)), name
        heads = [int(l[2]) for l in lines if l[0] == "head" and l[1] == name + ".dat"]
        assert heads == (list(np.array([135.523, 34.823, 120.5]).astype(F32).view(np.int32)) if head else []), name
        assert [l[2] for l in lines if l[0] == "end" and l[1] == name + ".dat"] == ["T"], name


def test_big_endian_is_the_byte_swap_of_every_word():
    rec = values(8)
    le, be = O.frame(rec, False, head=(1, 2, 3)), O.frame(rec, True, head=(1, 2, 3))
    assert np.array_equal(np.frombuffer(le, dtype="<u4"), np.frombuffer(be, dtype=">u4"))
    assert be[:4] == b"\x00\x00\x00\x04" and le[:4] == b"\x04\x00\x00\x00"
    assert O.same_bits(O.unframe(be, 8, True, head=True)[0], rec)


def one_row(elm, **kw):
    rec = np.zeros((1, 8), dtype=F32)
    rec[0, 0] = elm
    for k, v in kw.items():
        rec[0, {"lon": 1, "lat": 2, "lev": 3, "dat": 4, "err": 5, "typ": 6, "dif": 7}[k]] = v
    return rec


def test_the_single_precision_points_by_hand():
    # float32(1013.25) * 100.0f: 1013.25 is exact, the product 101325 is exact
    assert O.decode_obs(one_row(O.ID["u"], lev=1013.25), O.CONV)["lev"][0] == 101325.0
    # an RH of float32(55.5) * 0.01f: 0.01f = 0x3C23D70A = 0.00999999977648258209228515625; the product 0.554999987594783306..
    # rounds to the float32 0x3F0E147B = 0.555000007152557373046875, while the double product 55.5 * 0.01 = 0.555 rounds to the
    # float32 0x3F0E147B too but is, as a double, 0.555: the widened single is not the double
    rh = O.decode_obs(one_row(O.ID["rh"], dat=55.5), O.CONV)["dat"][0]
    assert rh == float(np.frombuffer(np.uint32(0x3F0E147B).tobytes(), dtype=F32)[0]) == 0.555000007152557373046875
    assert rh != 55.5 * 0.01 and rh != np.float64(F32(55.5)) * np.float64(F32(0.01))
    # 1e-37f * 0.01f is a denormal (below 2^-126 = 1.1754944e-38) and is kept: 1e-39 to single precision of its 2^-149 steps
    den = O.decode_obs(one_row(O.ID["rh"], err=1e-37), O.CONV)["err"][0]
    assert 0.0 < den < O.TINY and round(den / 2.0 ** -149) == den / 2.0 ** -149 and abs(den - 1e-39) <= 2.0 ** -149
    # NINT: half away from zero; NaN 0; saturation
    assert [O.nint(F32(v)) for v in (0.5, -0.5, 2.5, -2.5, 1.5, 0.49999997)] == [1, -1, 3, -3, 2, 0]
    assert O.nint(F32(np.nan)) == 0 and O.nint(F32(3e9)) == 2 ** 31 - 1 and O.nint(F32(-3e9)) == -2 ** 31
    # idx = 2^24 + 1 comes back as 2^24 ("will overflow")
    rec = O.encode_obsda([1], [2 ** 24 + 1], [0.0], [0])
    assert rec[0, 1] == 2.0 ** 24 and O.nint(rec[0, 1]) == 2 ** 24
    assert O.assemble([rec], [0], np.zeros((1, 1)), np.zeros(1, dtype=np.int32))["idx"][0] == 2 ** 24
    # dat equal to undef is left out; one float32 step off, and float32(undef) itself, are written
    step = float(np.nextafter(F32(O.UNDEF), F32(0.0)))
    cols = O.decode_obs(np.repeat(one_row(O.UNKNOWN_ID), 3, axis=0), O.CONV)
    cols["dat"][:] = [O.UNDEF, step, float(F32(O.UNDEF))]
    out = O.encode_obs(cols, O.CONV, 8, missing=False)
    assert len(out) == 2 and out[0, 4] == F32(step) and out[1, 4] == F32(O.UNDEF)
    assert len(O.encode_obs(cols, O.CONV, 8, missing=True)) == 3


def test_encode_is_the_inverse_where_nothing_is_scaled_and_the_reference_elsewhere():
    rec = O.conv_records(44, seed=2, tc=False)
    cols = O.decode_obs(rec, O.CONV)
    back = O.encode_obs(cols, O.CONV, 8)
    plain = cols["elm"] == O.UNKNOWN_ID
    assert plain.sum() >= 4 and O.same_bits(back[plain], rec[plain])
    # a scaled row: x * 100.0f * 0.01f in float32, not always x
    u = cols["elm"] == O.ID["u"]
    assert O.same_bits(back[u, 3], (rec[u, 3] * F32(100.0)) * F32(0.01))
    sym = cols["elm"] != O.ID["tcmip"]          # (read_obs scales a TC pressure row's level and replaces its error; write_obs does neither)
    assert np.allclose(back[sym], rec[sym], rtol=3e-7, atol=0.0) and not np.allclose(back[~sym], rec[~sym], rtol=3e-7, atol=0.0)
    radar = O.radar_records(20, 7)
    assert O.same_bits(O.encode_obs(O.decode_obs(radar, O.RADAR), O.RADAR, 7)[:, :6], radar[:, :6])


def test_the_departure_record_gathers_the_file_row():
    cols = O.decode_obs(O.conv_records(30, seed=9, tc=False), O.CONV)
    off = np.array([0, 10, 30])
    set_, idx = np.array([2, 1, 2]), np.array([20, 1, 3])
    rec = O.encode_dep(set_, idx, np.array([0, 10, 0]), np.array([0.5, -1.25, 3.0]), np.array([0.25, 2.0, -1.0]), off, cols)
    assert rec.shape == (3, 11)
    assert O.same_bits(rec[:, :8], O.encode_obs({k: v[[29, 0, 12]] for k, v in cols.items()}, O.CONV, 8))
    assert rec[:, 8].tolist() == [0.0, 10.0, 0.0] and rec[:, 9].tolist() == [0.5, -1.25, 3.0] and rec[:, 10].tolist() == [0.25, 2.0, -1.0]
