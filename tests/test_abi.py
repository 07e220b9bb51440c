"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports every
function include/letkf_amd.h declares; the Python binding's signature table, struct mirrors and option numbers are
the header's (read through tests/_header.py).  No compute call is made (there is no GPU here)."""
import ctypes as C

import pytest

import _header
from __graft_entry__ import load_package

# every argument struct of the header and its ctypes mirror
MIRRORS = {
    "letkf_core_batch_args": "CoreBatchArgs", "letkf_das_args": "DasArgs", "letkf_search_tables": "SearchTables",
    "letkf_state_consts": "StateConsts", "letkf_qc_params": "QcParams", "letkf_mesh": "Mesh",
    "letkf_halo_layout": "HaloLayout", "letkf_beta_params": "BetaParams", "letkf_setobs_params": "SetObsParams",
    "letkf_obs_file_rows": "ObsFileRows", "letkf_obs_table_info": "ObsTableInfo", "letkf_efso_args": "EfsoArgs",
    "letkf_das_obs_args": "DasObsArgs", "letkf_efso_norm_params": "EfsoNormParams",
}


@pytest.fixture(scope="module")
def pkg():
    p = load_package()
    p.build()
    return p


def test_header_symbols_exported(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    names = sorted(_header.entries())
    assert "letkf_core_c" in names and "letkf_das_points_dev" in names and len(names) >= 16
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/letkf_amd.h but not exported"
    assert set(names) == set(pkg.EXPORTS), "python binding list out of sync with the header"


def test_abi_version(pkg):
    assert pkg.lib().letkf_amd_abi_version() == _header.defines()["LETKF_AMD_ABI_VERSION"]


def test_fails_loudly_without_device(pkg):
    """No CPU fallback: creating a context without a GPU is an error, not a silent slow path."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.LetkfError):
        pkg.Context(0)


def test_every_entry_is_typed_as_the_header_declares(pkg):
    """Signatures: the binding's table, and what lib() set on the loaded functions, entry by entry in the header's order."""
    lib = pkg.lib()
    entries = _header.entries()
    assert len(entries) == 59
    wrong = []
    for name in entries:
        want, f = _header.argtypes_of(name), getattr(lib, name)
        want_res = {"letkf_amd_last_error": C.c_char_p, "letkf_core_c": None}.get(name, C.c_int)
        assert _header.restype_of(name) is want_res, name
        if pkg.ARGTYPES.get(name) != want or f.argtypes != want or f.restype is not want_res:   # (untyped: argtypes is None)
            wrong.append(name)
    assert not wrong, f"{len(wrong)} entries not typed as the header declares them: {wrong}"
    assert list(pkg.ARGTYPES) == list(entries) and set(pkg.EXPORTS) == set(entries)


def test_every_struct_mirror_has_the_header_layout(pkg):
    """Layouts: field names in the header's order, each with the ctypes type of its C kind, at the size and offsets gcc gives."""
    structs = _header.structs()
    assert len(structs) == 14 and sum(len(f) for f in structs.values()) == 303
    assert set(structs) == set(MIRRORS), "a struct of the header has no ctypes mirror named here (or the other way round)"
    for cname, fields in structs.items():
        cls = getattr(pkg, MIRRORS[cname])
        assert [n for n, _ in cls._fields_] == [n for _, n, _ in fields], cname
        for (name, ctype), (kind, _, count) in zip(cls._fields_, fields):
            assert ctype is _header.field_ctype(kind, count), (cname, name, ctype)
            assert getattr(cls, name).offset == _header.offsetof(cname, name), (cname, name)
        assert C.sizeof(cls) == _header.sizeof(cname), cname


def test_struct_layout_matches_header(pkg):
    # sizes of the argument blocks as the C compiler lays them out (guards the ctypes mirror)
    for cname in ("letkf_core_batch_args", "letkf_das_args", "letkf_search_tables", "letkf_state_consts", "letkf_beta_params"):
        assert _header.sizeof(cname) == C.sizeof(getattr(pkg, MIRRORS[cname])), cname


def test_option_numbers_are_the_headers(pkg):
    opts = {n[len("LETKF_"):]: v for n, v in _header.defines().items() if n.startswith("LETKF_OPT_")}
    assert len(opts) == 6
    assert {n: getattr(pkg.Context, n) for n in dir(pkg.Context) if n.startswith("OPT_")} == opts


def test_a_float_for_an_int32_parameter_is_refused(pkg):
    """letkf_obs_target_var(int32_t elm), host only: ctypes refuses the call, the library is not entered"""
    with pytest.raises(C.ArgumentError):
        pkg.lib().letkf_obs_target_var(2.5)


def test_a_bare_int_reaches_an_int64_parameter_whole(pkg):
    """letkf_sched_plan_check(int64_t npts, ...), host only: 2**40 as a bare Python int is the int64 it is as a c_int64 (untyped, it
    would be cut to a 32-bit int)"""
    check = pkg.lib().letkf_sched_plan_check
    rest = (1, 16, 512, 4, 256)
    assert check(2 ** 40, *rest) == check(C.c_int64(2 ** 40), *rest)
    assert check(2 ** 40, *rest) != check(0, *rest) == 0        # (more runs than the self-check walks: refused; its low 32 bits: none)
