"""CPU-only: the build recipe of torch_cfd_amd._lib.  The JOBS table is consistent with SOURCES and csrc/, and
build_library issues exactly the compiles and the link the table describes -- checked with a stub in place of hipcc that
records its arguments and touches its output.  Nothing here compiles or loads a library."""
import json
import os
import shutil
import stat
import sys

import pytest

from torch_cfd_amd import _lib

COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]


def test_every_job_source_is_listed_and_exists():
    for src, _, _ in _lib.JOBS:
        assert src in _lib.SOURCES, src
        assert os.path.isfile(os.path.join(_lib.CSRC, src)), src


def test_every_source_has_a_job():
    assert set(_lib.SOURCES) == {src for src, _, _ in _lib.JOBS}
    assert len(set(_lib.SOURCES)) == len(_lib.SOURCES)


def test_objects_are_unique_and_jobs_fit_the_build_cpus():
    objs = [obj for _, _, obj in _lib.JOBS]
    assert len(set(objs)) == len(objs)
    assert all(o.endswith(".o") and os.path.basename(o) == o for o in objs)
    assert len(_lib.JOBS) <= 16


def test_a_source_appears_twice_only_with_different_flags():
    seen = [(src, tuple(flags)) for src, flags, _ in _lib.JOBS]
    assert len(set(seen)) == len(seen)


STUB = """#!{python}
import json, os, sys
line = (json.dumps(sys.argv[1:]) + "\\n").encode()
fd = os.open({log!r}, os.O_WRONLY | os.O_CREAT | os.O_APPEND, 0o644)
os.write(fd, line)
os.close(fd)
open(sys.argv[sys.argv.index("-o") + 1], "w").close()
"""


@pytest.fixture
def stub_build(tmp_path, monkeypatch):
    """_lib pointed at a copy of csrc/ (sources and headers only) and at a recording stub compiler; returns (csrc, calls)."""
    csrc = tmp_path / "csrc"
    csrc.mkdir()
    for f in os.listdir(_lib.CSRC):
        if f.endswith((".hip", ".hpp")):
            shutil.copy(os.path.join(_lib.CSRC, f), csrc / f)
    log = tmp_path / "hipcc.log"
    stub = tmp_path / "hipcc_stub"
    stub.write_text(STUB.format(python=sys.executable, log=str(log)))
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setenv("HIPCC", str(stub))
    monkeypatch.setattr(_lib, "CSRC", str(csrc))
    monkeypatch.setattr(_lib, "LIB_PATH", str(csrc / _lib.LIB_NAME))

    def calls():
        got = [json.loads(line) for line in log.read_text().splitlines()] if log.exists() else []
        return [c for c in got if "-c" in c], [c for c in got if "-shared" in c]

    return str(csrc), calls


def expected_compile(csrc, job):
    src, flags, obj = job
    return COMMON + list(flags) + ["-c", os.path.join(csrc, src), "-o", os.path.join(csrc, obj)]


def linked_objects(link):
    return [a for a in link if a.endswith(".o")]


def test_full_build_compiles_every_job_once_and_links_their_objects(stub_build):
    csrc, calls = stub_build
    path = _lib.build_library(force=True)
    compiles, links = calls()
    assert sorted(compiles) == sorted(expected_compile(csrc, job) for job in _lib.JOBS)
    assert len(links) == 1
    assert linked_objects(links[0]) == [os.path.join(csrc, obj) for _, _, obj in _lib.JOBS]
    assert path == os.path.join(csrc, _lib.LIB_NAME) and os.path.exists(path)
    assert not [f for f in os.listdir(csrc) if ".tmp" in f]


def test_only_recompiles_the_named_source_and_links_everything(stub_build):
    csrc, calls = stub_build
    _lib.build_library(force=True)
    before = calls()
    _lib.build_library(only=["tcfd_loss.hip"])
    compiles, links = calls()
    new_compiles, new_links = compiles[len(before[0]):], links[len(before[1]):]
    assert new_compiles == [expected_compile(csrc, job) for job in _lib.JOBS if job[0] == "tcfd_loss.hip"]
    assert len(new_links) == 1
    assert linked_objects(new_links[0]) == [os.path.join(csrc, obj) for _, _, obj in _lib.JOBS]


def test_only_names_every_job_of_a_source_compiled_twice(stub_build):
    csrc, calls = stub_build
    _lib.build_library(force=True)
    n = len(calls()[0])
    _lib.build_library(only=("tcfd_ns2d_sized.hip",))
    assert sorted(calls()[0][n:]) == sorted(expected_compile(csrc, job) for job in _lib.JOBS if job[0] == "tcfd_ns2d_sized.hip")


def test_only_raises_when_another_object_is_absent(stub_build):
    csrc, calls = stub_build
    with pytest.raises(_lib.TcfdError, match="tcfd_fvm.o"):      # nothing built yet: every other object is missing
        _lib.build_library(only=["tcfd_loss.hip"])
    assert calls() == ([], [])                                   # and nothing was started
    _lib.build_library(force=True)
    os.remove(os.path.join(csrc, "tcfd_grf.o"))
    n = len(calls()[0])
    with pytest.raises(_lib.TcfdError, match="tcfd_grf.o"):
        _lib.build_library(only=["tcfd_loss.hip"])
    assert len(calls()[0]) == n


def test_only_raises_for_an_unknown_name(stub_build):
    _, calls = stub_build
    with pytest.raises(_lib.TcfdError, match="no_such_unit.hip"):
        _lib.build_library(only=["tcfd_loss.hip", "no_such_unit.hip"])
    assert calls() == ([], [])
