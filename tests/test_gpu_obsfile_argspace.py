"""The record codec's entries (include/letkf_amd_obsfile.h) across their argument space: every refusal the header lists, once
each, with LETKF_E_INVALID, an error text that names the argument and nothing written (the outputs keep their canary); and every
optional output NULL in turn, the others unchanged by it."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _header
import _obsfile as O

pytestmark = pytest.mark.gpu
E_INVALID = _header.defines()["LETKF_E_INVALID"]
N, NMEM, KLD = 70, 3, 5
CANARY = 0xA5
DEFAULT = object()                         # "the valid argument"; None is NULL


@pytest.fixture(scope="module")
def env():
    from _gpu import ctx, pkg
    return pkg, ctx()


def canary(nbytes):
    return torch.full((nbytes + 8,), CANARY, dtype=torch.uint8, device="cuda")


def untouched(*tensors):
    torch.cuda.synchronize()
    return all(bool((t == CANARY).all().item()) for t in tensors)


class Call:
    """the arguments of one valid call of every entry, rebuilt per test: change one, call, expect the refusal"""

    def __init__(self, pkg, ctx):
        self.pkg, self.c, self.lib = pkg, ctx._c, pkg.obsfile_lib()
        rec = O.conv_records(N, seed=1, tc=False)
        self.image = torch.from_numpy(np.frombuffer(O.frame(rec), dtype=np.uint8).copy()).cuda()
        self.radar = torch.from_numpy(np.frombuffer(O.frame(O.radar_records(N, 7), head=(1, 2, 3)), dtype=np.uint8).copy()).cuda()
        self.cols_out = {k: canary(N * 8) for k in O.COLUMNS}
        st = O.decode_obs(rec, O.CONV)
        self.cols_in = {k: torch.from_numpy(st[k]).cuda() for k in O.COLUMNS}
        self.image_out = canary(N * 40)
        recs = O.obsda_records(N, NMEM, 4)
        self.das = [torch.from_numpy(np.frombuffer(O.frame(r), dtype=np.uint8).copy()).cuda() for r in recs]
        self.da_out = dict(set=canary(N * 4), idx=canary(N * 4), qc=canary(N * 4), ensval=canary(N * KLD * 8), lev=canary(N * 8), val2=canary(N * 8))
        self.i32 = {k: torch.ones(N, dtype=torch.int32, device="cuda") for k in ("set", "idx", "qc")}
        self.f64 = {k: torch.zeros(N, dtype=torch.float64, device="cuda") for k in ("omb", "oma", "val", "lev", "val2")}
        self.ens = torch.zeros((N, KLD), dtype=torch.float64, device="cuda")
        self.off = np.array([0, 30, N], dtype=np.int64)
        self.badproj = pkg.Mapproj()
        self.badproj.type = 2
        self.outputs = list(self.cols_out.values()) + [self.image_out] + list(self.da_out.values())

    # -- the structs
    def params(self, **kw):
        p = self.pkg.ObsfileParams()
        p.format, p.nrec, p.missing = O.CONV, 8, 1
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def cols(self, src, **kw):
        o = self.pkg.ObsfileCols()
        for k in O.COLUMNS:
            setattr(o, k, kw[k] if k in kw else src[k].data_ptr())
        return o

    def da_params(self, **kw):
        p = self.pkg.ObsdaParams()
        p.nrec, p.nmem, p.nobs, p.kld = 4, NMEM, N, KLD
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def da_cols(self, **kw):
        o = self.pkg.ObsdaCols()
        for k, _ in o._fields_:
            setattr(o, k, kw[k] if k in kw else self.da_out[k].data_ptr())
        return o

    def rows(self, **kw):
        f = self.pkg.ObsfileRows()
        f.nfile, f.off = 2, self.off.ctypes.data
        for k in O.COLUMNS:
            setattr(f, k, self.cols_in[k].data_ptr())
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    # -- the entries; every keyword replaces one argument
    def decode(self, p=DEFAULT, image="conv", nrows=N, o=DEFAULT, proj=None, nbad=None, meta=None, ctx=DEFAULT):
        p = self.params() if p is DEFAULT else p
        img = {"conv": self.image.data_ptr(), "radar": self.radar.data_ptr()}.get(image, image)
        o = self.cols(self.cols_out) if o is DEFAULT else o
        return self.lib.letkf_obs_decode_dev(self.c if ctx is DEFAULT else ctx, None if p is None else C.addressof(p), proj, img, nrows,
                                             None if o is None else C.addressof(o), meta, nbad)

    def encode(self, p=None, nrows=N, cin=None, meta=None, image=None, nwritten=None):
        p = p if p is not None else self.params()
        cin = cin if cin is not None else self.cols(self.cols_in)
        return self.lib.letkf_obs_encode_dev(self.c, C.addressof(p), nrows, C.addressof(cin), meta,
                                             self.image_out.data_ptr() if image is None else image, nwritten)

    def assemble(self, p=None, images=None, col=(0, 1, 2), is_member=None, o=None, ninc=None, nbad=None):
        p = p if p is not None else self.da_params()
        ptrs = (C.c_void_p * 3)(*(images if isinstance(images, list) else [t.data_ptr() for t in self.das]))
        colv = None if col is None else np.array(col, dtype=np.int32)
        o = o if o is not None else self.da_cols()
        return self.lib.letkf_obsda_assemble_dev(self.c, C.addressof(p), None if images == "null" else C.addressof(ptrs),
                                                 None if colv is None else colv.ctypes.data, is_member, C.addressof(o), ninc, nbad)

    def da_encode(self, nrec=4, nobs=N, kld=KLD, col=0, image=None, **kw):
        a = dict(set=self.i32["set"].data_ptr(), idx=self.i32["idx"].data_ptr(), qc=self.i32["qc"].data_ptr(), ensval=self.ens.data_ptr(),
                 val=self.f64["val"].data_ptr(), lev=self.f64["lev"].data_ptr(), val2=self.f64["val2"].data_ptr())
        a.update(kw)
        return self.lib.letkf_obsda_encode_dev(self.c, nrec, 0, nobs, a["set"], a["idx"], a["qc"], a["ensval"], kld, col, a["val"], a["lev"],
                                               a["val2"], self.image_out.data_ptr() if image is None else image)

    def dep(self, nobs=N, files=None, image=None, **kw):
        a = dict(set=self.i32["set"].data_ptr(), idx=self.i32["idx"].data_ptr(), qc=self.i32["qc"].data_ptr(), omb=self.f64["omb"].data_ptr(),
                 oma=self.f64["oma"].data_ptr())
        a.update(kw)
        f = files if files is not None else self.rows()
        return self.lib.letkf_obsdep_encode_dev(self.c, 0, nobs, a["set"], a["idx"], a["qc"], a["omb"], a["oma"], C.addressof(f),
                                                self.image_out.data_ptr() if image is None else image)


REFUSALS = {
    # NULL required pointers
    "decode_params_null": (lambda k: k.decode(p=None), "params"),
    "decode_o_null": (lambda k: k.decode(o=None), "o is NULL"),
    "decode_image_null": (lambda k: k.decode(image=0), "image"),
    "decode_ctx_null": (lambda k: k.decode(ctx=None), "ctx"),
    "decode_proj_null_but_given": (lambda k: k.decode(p=k.params(proj_given=1)), "proj"),
    "decode_proj_of_another_type": (lambda k: k.decode(p=k.params(proj_given=1), proj=C.addressof(k.badproj)), "proj->type"),
    "encode_column_null": (lambda k: k.encode(cin=k.cols(k.cols_in, err=None)), "err"),
    "encode_dif_null_nrec8": (lambda k: k.encode(cin=k.cols(k.cols_in, dif=None)), "dif"),
    "encode_image_null": (lambda k: k.encode(image=0), "image"),
    "encode_nwritten_null_without_missing": (lambda k: k.encode(p=k.params(missing=0)), "nwritten"),
    "encode_radar_meta_null": (lambda k: k.encode(p=k.params(format=O.RADAR, nrec=7)), "meta"),
    "assemble_images_null": (lambda k: k.assemble(images="null"), "images"),
    "assemble_col_null": (lambda k: k.assemble(col=None), "col"),
    "assemble_one_image_null": (lambda k: k.assemble(images=[k.das[0].data_ptr(), 0, k.das[2].data_ptr()]), r"images\[1\]"),
    "assemble_ensval_null": (lambda k: k.assemble(o=k.da_cols(ensval=None)), "ensval"),
    "da_encode_set_null": (lambda k: k.da_encode(set=None), "set"),
    "da_encode_val_null_with_negative_col": (lambda k: k.da_encode(col=-1, val=None), "val"),
    "da_encode_lev_null_nrec6": (lambda k: k.da_encode(nrec=6, lev=None), "lev"),
    "dep_omb_null": (lambda k: k.dep(omb=None), "omb"),
    "dep_files_column_null": (lambda k: k.dep(files=k.rows(lat=None)), "files"),
    "dep_files_off_null": (lambda k: k.dep(files=k.rows(off=None)), "off"),
    # alignment
    "decode_image_unaligned": (lambda k: k.decode(image=k.image.data_ptr() + 2), "4-byte aligned"),
    "encode_image_unaligned": (lambda k: k.encode(image=k.image_out.data_ptr() + 1), "4-byte aligned"),
    "assemble_image_unaligned": (lambda k: k.assemble(images=[k.das[0].data_ptr(), k.das[1].data_ptr(), k.das[2].data_ptr() + 3]), r"images\[2\]"),
    "da_encode_image_unaligned": (lambda k: k.da_encode(image=k.image_out.data_ptr() + 2), "4-byte aligned"),
    "dep_image_unaligned": (lambda k: k.dep(image=k.image_out.data_ptr() + 1), "4-byte aligned"),
    # format and nrec
    "decode_format_obsda": (lambda k: k.decode(p=k.params(format=O.OBSDA, nrec=4)), "format"),
    "decode_conv_nrec7": (lambda k: k.decode(p=k.params(nrec=7)), "nrec"),
    "decode_radar_nrec6": (lambda k: k.decode(p=k.params(format=O.RADAR, nrec=6), image="radar"), "nrec"),
    "encode_format_0": (lambda k: k.encode(p=k.params(format=0)), "format"),
    "assemble_nrec5": (lambda k: k.assemble(p=k.da_params(nrec=5)), "nrec"),
    "da_encode_nrec8": (lambda k: k.da_encode(nrec=8), "nrec"),
    # counts
    "decode_nrows_negative": (lambda k: k.decode(nrows=-1), "nrows"),
    "decode_nrows_2_31": (lambda k: k.decode(nrows=2 ** 31), "nrows"),
    "encode_nrows_negative": (lambda k: k.encode(nrows=-1), "nrows"),
    "assemble_nobs_negative": (lambda k: k.assemble(p=k.da_params(nobs=-1)), "nobs"),
    "assemble_nmem_0": (lambda k: k.assemble(p=k.da_params(nmem=0)), "nmem"),
    "assemble_nmem_above": (lambda k: k.assemble(p=k.da_params(nmem=65537)), "nmem"),
    "assemble_kld_0": (lambda k: k.assemble(p=k.da_params(kld=0)), "kld"),
    "assemble_kld_2_20": (lambda k: k.assemble(p=k.da_params(kld=2 ** 20)), "kld"),
    "assemble_member_0_with_finish": (lambda k: k.assemble(p=k.da_params(nrec=6, finish=1, member=0)), "member"),
    "da_encode_nobs_negative": (lambda k: k.da_encode(nobs=-5), "nobs"),
    "da_encode_col_beyond_kld": (lambda k: k.da_encode(col=KLD), "col"),
    "dep_nobs_negative": (lambda k: k.dep(nobs=-1), "nobs"),
    "dep_nfile_negative": (lambda k: k.dep(files=k.rows(nfile=-1)), "nfile"),
    # col
    "assemble_col_negative": (lambda k: k.assemble(col=(0, -1, 2)), r"col\[1\]"),
    "assemble_col_kld": (lambda k: k.assemble(col=(0, 1, KLD)), r"col\[2\]"),
    "assemble_col_repeated": (lambda k: k.assemble(col=(4, 1, 4)), r"col\[2\] repeats"),
    # overlap
    "decode_output_on_the_image": (lambda k: k.decode(o=k.cols(k.cols_out, lat=k.image.data_ptr() + 8)), "lat overlaps image"),
    "decode_output_on_an_output": (lambda k: k.decode(o=k.cols(k.cols_out, lev=k.cols_out["dat"].data_ptr() + 16)), "lev overlaps dat"),
    "encode_image_on_an_input": (lambda k: k.encode(image=k.cols_in["lon"].data_ptr()), "image overlaps lon"),
    "assemble_ensval_on_an_image": (lambda k: k.assemble(o=k.da_cols(ensval=k.das[1].data_ptr())), r"ensval overlaps images\[1\]"),
    "assemble_qc_on_set": (lambda k: k.assemble(o=k.da_cols(qc=k.da_out["set"].data_ptr() + 4)), "overlaps"),
    "da_encode_image_on_ensval": (lambda k: k.da_encode(image=k.ens.data_ptr()), "image overlaps ensval"),
    "dep_image_on_a_file_column": (lambda k: k.dep(image=k.cols_in["dat"].data_ptr()), "image overlaps files->dat"),
}


@pytest.mark.parametrize("name", list(REFUSALS))
def test_refused_with_nothing_written(env, name):
    pkg, ctx = env
    k = Call(pkg, ctx)
    call, word = REFUSALS[name]
    before = {n: t.clone() for n, t in k.cols_in.items()}
    assert call(k) == E_INVALID, name
    assert re.search(word, pkg.lib().letkf_amd_last_error().decode()), pkg.lib().letkf_amd_last_error().decode()
    assert untouched(*k.outputs), name
    assert all(torch.equal(before[n], k.cols_in[n]) for n in before)


@pytest.mark.parametrize("what,row,value", [("set", 0, 0), ("set", 69, 3), ("idx", 5, 0), ("idx", 7, 31), ("idx", 40, -2)])
def test_a_departure_row_outside_the_files_is_refused_before_anything_is_written(env, what, row, value):
    pkg, ctx = env
    k = Call(pkg, ctx)
    k.i32["set"][40:] = 2                                 # file 2 has 40 rows, file 1 has 30
    k.i32["idx"][:] = 30
    k.i32[what][row] = value
    assert k.dep() == E_INVALID
    assert "1 rows have a set / idx outside the files" in pkg.lib().letkf_amd_last_error().decode()
    assert untouched(*k.outputs)
    k.i32[what][row] = 1
    assert k.dep() == 0 and not untouched(k.image_out)


def test_the_host_entries_refuse(env):
    pkg, _ = env
    lib, n = pkg.obsfile_lib(), C.c_int64(77)
    for fmt, nrec, nbytes in ((O.CONV, 8, 41), (O.CONV, 8, -40), (O.RADAR, 7, 35), (O.RADAR, 7, 36 + 35), (O.RADAR, 9, 36), (O.OBSDA, 5, 0),
                              (O.DEP, 10, 0), (0, 8, 40), (5, 8, 40)):
        assert lib.letkf_obsfile_count(fmt, nrec, nbytes, C.addressof(n)) == E_INVALID and n.value == 77, (fmt, nrec, nbytes)
    assert lib.letkf_obsfile_count(O.CONV, 8, 40, None) == E_INVALID
    assert lib.letkf_obsfile_bytes(O.CONV, 8, -1, C.addressof(n)) == E_INVALID and lib.letkf_obsfile_bytes(O.CONV, 8, 1, None) == E_INVALID
    for fmt, nrec, head in ((O.CONV, 8, 0), (O.RADAR, 7, 36), (O.RADAR, 8, 36), (O.OBSDA, 4, 0), (O.OBSDA, 6, 0), (O.DEP, 11, 0)):
        for rows in (0, 1, 1000):
            assert pkg.obsfile_bytes(fmt, nrec, rows) == head + rows * 4 * (nrec + 2)
            assert pkg.obsfile_count(fmt, nrec, head + rows * 4 * (nrec + 2)) == rows == O.count(fmt, nrec, head + rows * 4 * (nrec + 2))


def test_zero_rows_is_no_error(env):
    pkg, ctx = env
    k = Call(pkg, ctx)
    nw = C.c_int64(-1)
    assert k.decode(nrows=0, image=0) == 0
    assert k.encode(nrows=0, p=k.params(missing=0), nwritten=C.addressof(nw)) == 0 and nw.value == 0
    assert k.assemble(p=k.da_params(nobs=0)) == 0
    assert k.da_encode(nobs=0) == 0 and k.dep(nobs=0) == 0
    assert untouched(*k.outputs)


@pytest.mark.parametrize("absent", O.COLUMNS + ("nbad",))
def test_every_optional_output_of_the_decoder_may_be_null(env, absent):
    pkg, ctx = env
    k = Call(pkg, ctx)
    full = {n: torch.zeros(N, dtype=torch.int32 if n in ("elm", "typ") else torch.float64, device="cuda") for n in O.COLUMNS}
    nbad = C.c_int64(-1)
    assert k.decode(o=k.cols(full), nbad=C.addressof(nbad)) == 0 and nbad.value == 0
    part = {n: torch.zeros_like(t) for n, t in full.items()}
    o = k.cols(part, **({absent: None} if absent != "nbad" else {}))
    assert k.decode(o=o, nbad=None if absent == "nbad" else C.addressof(nbad)) == 0
    torch.cuda.synchronize()
    for n in O.COLUMNS:
        if n == absent:
            assert not part[n].any()
        else:
            assert torch.equal(part[n].view(torch.uint8), full[n].view(torch.uint8)), n


@pytest.mark.parametrize("absent", ["ninconsistent", "nbad", "both", "is_member", "lev", "val2"])
def test_every_optional_argument_of_the_assembler_may_be_null(env, absent):
    pkg, ctx = env
    nrec = 6 if absent in ("lev", "val2", "is_member") else 4
    recs = O.obsda_records(N, NMEM, nrec)
    images = [torch.from_numpy(np.frombuffer(O.frame(r), dtype=np.uint8).copy()).cuda() for r in recs]
    st = O.assemble(recs, np.arange(NMEM), np.zeros((N, NMEM)), np.zeros(N, dtype=np.int32), None, np.zeros(N), np.zeros(N))
    out = {n: torch.zeros(N, dtype=torch.int32, device="cuda") for n in ("set", "idx", "qc")}
    out["ensval"] = torch.zeros((N, NMEM), dtype=torch.float64, device="cuda")
    out["lev"], out["val2"] = (None if absent == n else torch.zeros(N, dtype=torch.float64, device="cuda") for n in ("lev", "val2"))
    p = pkg.ObsdaParams()
    p.nrec, p.nmem, p.nobs, p.kld = nrec, NMEM, N, NMEM
    o = pkg.ObsdaCols()
    for n, _ in o._fields_:
        setattr(o, n, None if out[n] is None else out[n].data_ptr())
    ptrs, col = (C.c_void_p * NMEM)(*[t.data_ptr() for t in images]), np.arange(NMEM, dtype=np.int32)
    flags = np.ones(NMEM, dtype=np.int32)
    ninc, nbad = C.c_int64(-1), C.c_int64(-1)
    rc = pkg.obsfile_lib().letkf_obsda_assemble_dev(ctx._c, C.addressof(p), C.addressof(ptrs), col.ctypes.data,
                                                    None if absent == "is_member" else flags.ctypes.data, C.addressof(o),
                                                    None if absent in ("ninconsistent", "both") else C.addressof(ninc),
                                                    None if absent in ("nbad", "both") else C.addressof(nbad))
    assert rc == 0, pkg.lib().letkf_amd_last_error().decode()
    torch.cuda.synchronize()
    assert ninc.value == (-1 if absent in ("ninconsistent", "both") else 0) and nbad.value == (-1 if absent in ("nbad", "both") else 0)
    for n in ("set", "idx", "qc", "ensval") + (("lev", "val2") if nrec == 6 else ()):
        if out[n] is not None:
            assert O.same_bits(out[n].cpu().numpy(), st[n]), n
