"""ops._launch - the one path from the host operators onto the device - against a stub library and a stub stream (no GPU), and
the storage suffix table against the declared C ABI."""
import pytest
import torch

import vipcup_amd  # noqa: F401
from vipcup_amd import _abi, ops

STREAM = object()


class StubLib:
    def __init__(self, log, status=0):
        self.log, self.status = log, status

    def __getattr__(self, name):
        if not name.startswith("vip_"):
            raise AttributeError(name)

        def call(*args):
            self.log.append(("call", name, args))
            return self.status
        return call

    def vip_last_error(self):
        return b"stub error"


class StubProf:
    def __init__(self, log):
        self.log = log

    def start(self, kernel, flops, nbytes, tag=None):
        self.log.append(("start", kernel, flops, nbytes, tag))
        return len(self.log)

    def stop(self, tok):
        self.log.append(("stop", tok))


@pytest.fixture
def stub(monkeypatch):
    log = []
    lib = StubLib(log)
    word = torch.zeros((1,), dtype=torch.int32)
    monkeypatch.setattr(_abi, "lib", lambda: lib)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    monkeypatch.setattr(ops, "h2_status", lambda device=None: word)
    monkeypatch.setattr(ops, "_PROF", None)
    return lib, log, word


def test_launch_appends_status_then_stream(stub):
    _, log, word = stub
    ops._launch("vip_layernorm_h2", 1, 2.5, status=True)
    ops._launch("vip_layernorm_s32", 1, 2.5)
    (_, n0, a0), (_, n1, a1) = log
    assert (n0, n1) == ("vip_layernorm_h2", "vip_layernorm_s32")
    assert a0[:2] == (1, 2.5) and a0[2].value == word.data_ptr() and a0[3] is STREAM and len(a0) == 4
    assert a1 == (1, 2.5, STREAM)


def test_launch_brackets_the_call_only_under_a_profiler(stub, monkeypatch):
    _, log, _ = stub
    monkeypatch.setattr(ops, "_PROF", StubProf(log))
    ops._launch("vip_mul_f16", 7, prof=lambda: ("mul_kernel", 1.0, 2.0, "tag"))
    ops._launch("vip_mul_f16", 8, prof=lambda: ("mul_kernel", 1.0, 2.0))       # the tag is optional
    ops._launch("vip_mul_f16", 9)                                              # nothing to report: not bracketed
    assert [e[0] for e in log] == ["start", "call", "stop", "start", "call", "stop", "call"]
    assert log[0] == ("start", "mul_kernel", 1.0, 2.0, "tag") and log[2] == ("stop", 1)
    assert log[3] == ("start", "mul_kernel", 1.0, 2.0, None) and log[5] == ("stop", 4)


def test_launch_never_evaluates_prof_without_a_profiler(stub):
    _, log, _ = stub

    def prof():
        raise AssertionError("prof evaluated with no profiler installed")
    ops._launch("vip_mul_f16", 7, prof=prof)
    assert [e[:2] for e in log] == [("call", "vip_mul_f16")]


def test_launch_error_names_the_symbol_it_called(stub):
    lib, _, _ = stub
    lib.status = 3
    with pytest.raises(_abi.VipError, match=r"^vip_radix_combine2_f16 failed with vip_status 3: stub error$"):
        ops._launch("vip_radix_combine2_f16", 1)


def test_launch_kind_resolves_suffix_and_status(stub):
    _, log, word = stub
    ops._launch_kind("cam", "f16", 1)
    ops._launch_kind("layernorm", "h2", 1)
    ops._launch_kind("gap_ln_dense", "h2", 1)
    assert [(e[1], len(e[2])) for e in log] == [("vip_cam_f32", 2), ("vip_layernorm_h2", 3), ("vip_gap_ln_dense_h2", 2)]
    assert log[1][2][1].value == word.data_ptr()


def test_suffix_table_matches_the_declared_abi():
    """every entry point the table can name is declared, takes the stream last, and the packed one carries exactly the status word
    more than its fp32-storage twin where the table says so"""
    for base, (suffix, status) in ops._KIND_OPS.items():
        assert {"s32", "h2"} <= set(suffix) <= {"f16", "s32", "h2"}, base
        sigs = {}
        for kind, sfx in suffix.items():
            name = f"vip_{base}_{sfx}"
            assert name in _abi.SIGNATURES, name
            sigs[kind] = _abi.SIGNATURES[name][1]
        assert sigs["h2"] == sigs["s32"][:-1] + [_abi._vp] * (1 + status), base
        if "f16" in sigs:
            assert sigs["f16"] == sigs["s32"], base
