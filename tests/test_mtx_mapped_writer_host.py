"""xck_write_mtx's two ways into the file (csrc/mtx_writer.cpp), without a GPU: the mapped path (XCK_WRITE_MAP=1: sizes first, the file
allocated at its final size and mapped, every thread formatting its chunks in place) against the pipeline (the default, and
XCK_WRITE_MAP=0: formatted into a ring of buffers, drained in file order), byte for byte, and both against the text Python formats line
by line (merge_mtx's format, rdr/fc/utils.py:54-93).  XCK_WRITE_CHUNK_ENTRIES makes tiny matrices span many chunks.  Reference
boundary: the file format; the reference writes it serially."""
import ctypes as C
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from xcltk_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = C.POINTER(C.c_int32)
INT32_MAX = 2**31 - 1
HEAD = b"%%MatrixMarket matrix coordinate integer general\n%%\n"


def _arrays(row, col, val, rm):
    return [np.ascontiguousarray(a, dtype=np.int32) for a in (row, col, val, rm)]


def _write(lib, path, row, col, val, rm, n_rows_out, n_cols):
    coo = capi.Coo(); coo.nnz = len(row)
    coo.row = row.ctypes.data_as(I32); coo.col = col.ctypes.data_as(I32); coo.val = val.ctypes.data_as(I32)
    return lib.xck_write_mtx(str(path).encode(), C.byref(coo), rm.ctypes.data_as(I32), n_rows_out, n_cols)


def _text(row, col, val, rm, n_rows_out, n_cols):
    r = rm[row]; k = r > 0
    body = b"".join(b"%d\t%d\t%d\n" % t for t in zip(r[k].tolist(), (col[k].astype(np.int64) + 1).tolist(), val[k].tolist()))
    return HEAD + b"%d\t%d\t%d\n" % (n_rows_out, n_cols, int(k.sum())) + body


def _both(lib, tmp_path, monkeypatch, row, col, val, rm, chunk, threads=3, n_rows_out=None, n_cols=77, stale=0):
    """The file with XCK_WRITE_MAP unset, 0 and 1 (over `stale` bytes of an older, longer file if asked): equal to each other and to
    Python's text; returns the bytes."""
    row, col, val, rm = _arrays(row, col, val, rm)
    n_rows_out = int(max(rm.max(), 0)) if n_rows_out is None else n_rows_out
    if chunk: monkeypatch.setenv("XCK_WRITE_CHUNK_ENTRIES", str(chunk))
    else: monkeypatch.delenv("XCK_WRITE_CHUNK_ENTRIES", raising=False)
    monkeypatch.setenv("XCK_WRITE_THREADS", str(threads))
    exp = _text(row, col, val, rm, n_rows_out, n_cols)
    got = {}
    for name, knob in (("default", None), ("pipeline", "0"), ("mapped", "1")):
        if knob is None: monkeypatch.delenv("XCK_WRITE_MAP", raising=False)
        else: monkeypatch.setenv("XCK_WRITE_MAP", knob)
        fn = tmp_path / (name + ".mtx")
        if stale: fn.write_bytes(b"#" * (len(exp) + stale))
        assert _write(lib, fn, row, col, val, rm, n_rows_out, n_cols) == 0, name
        got[name] = fn.read_bytes()
    assert got["mapped"] == got["pipeline"] and got["default"] == got["pipeline"]
    assert got["mapped"] == exp
    return got["mapped"]


def _random(n, n_rows, seed):
    rng = np.random.default_rng(seed)
    return np.sort(rng.integers(0, n_rows, n)), rng.integers(0, 5000, n), rng.integers(1, 300, n), np.arange(1, n_rows + 1)


@pytest.mark.parametrize("chunk", [7, 64])
@pytest.mark.parametrize("which", ["0", "1", "chunk-1", "chunk", "chunk+1", "many"])
def test_sizes_around_the_chunk(lib, tmp_path, monkeypatch, chunk, which):
    n = {"0": 0, "1": 1, "chunk-1": chunk - 1, "chunk": chunk, "chunk+1": chunk + 1, "many": 9 * chunk + 3}[which]
    out = _both(lib, tmp_path, monkeypatch, *_random(n, 12, seed=n), chunk=chunk)
    assert out.split(b"\n")[2] == b"12\t77\t%d" % n and out.count(b"\n") == 3 + n          # the header's counts


def test_one_row_run_across_several_chunks(lib, tmp_path, monkeypatch):
    n = 5 * 7 + 3
    rng = np.random.default_rng(3)
    out = _both(lib, tmp_path, monkeypatch, np.full(n, 2), np.sort(rng.integers(0, 10**6, n)), rng.integers(1, 9, n), [5, 6, 123456], chunk=7)
    assert all(l.startswith(b"123456\t") for l in out.split(b"\n")[3:-1])


@pytest.mark.parametrize("case", ["some", "last-chunk", "all"])
def test_row_map_drops_rows(lib, tmp_path, monkeypatch, case):
    n, chunk = 64, 7                                           # ten chunks, the last of one entry
    row = np.repeat(np.arange(16), 4)
    rm = np.arange(1, 17)
    if case == "some": rm[[0, 5, 6, 11]] = [0, -1, 0, -7]      # <= 0: not written
    if case == "last-chunk": rm[15] = 0                        # entries 60 - 63: the whole last chunk and the tail of the one before
    if case == "all": rm[:] = 0
    out = _both(lib, tmp_path, monkeypatch, row, np.arange(n), np.arange(1, n + 1), rm, chunk=chunk, n_rows_out=16)
    kept = int((rm[row] > 0).sum())
    assert out.split(b"\n")[2] == b"16\t77\t%d" % kept
    if case == "all": assert out == HEAD + b"16\t77\t0\n"


def test_numbers_of_every_width(lib, tmp_path, monkeypatch):
    """Values, columns and (through row_map) rows of 1 to 10 digits, INT32_MAX in each place, negative values."""
    edges = [1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 10**6, 10**7 - 1, 10**7, 10**8 - 1, 10**8, 10**9 - 1, 10**9, INT32_MAX]
    n = len(edges)
    val = edges + [-e for e in edges] + [-INT32_MAX - 1]
    col = [e - 1 for e in edges] + [e - 1 for e in reversed(edges)] + [0]              # col + 1 is written
    row = np.sort(np.arange(len(val)) % n)                                             # row r is written as edges[r]
    out = _both(lib, tmp_path, monkeypatch, row, col, val, edges, chunk=7, n_rows_out=INT32_MAX, n_cols=INT32_MAX)
    assert out.startswith(HEAD + b"2147483647\t2147483647\t%d\n" % len(val))
    assert b"\t-2147483648\n" in out and b"\t2147483647\t2147483647\n" in out and b"\n2147483647\t" in out     # value, column + value, row


@pytest.mark.parametrize("threads", [1, 3, 16])
def test_thread_counts(lib, tmp_path, monkeypatch, threads):
    _both(lib, tmp_path, monkeypatch, *_random(1000, 40, seed=threads), chunk=64, threads=threads)


def test_longer_file_already_there_leaves_no_tail(lib, tmp_path, monkeypatch):
    _both(lib, tmp_path, monkeypatch, *_random(500, 20, seed=8), chunk=64, stale=100000)
    _both(lib, tmp_path, monkeypatch, *_random(0, 20, seed=8), chunk=64, stale=5000)       # header only over an older file


@pytest.mark.parametrize("knob", [None, "1"])
def test_dev_null_and_fifo_take_the_pipeline(lib, tmp_path, monkeypatch, knob):
    """Neither is a regular file: nothing is allocated or mapped even where a mapping is asked for, the text goes through write calls in
    file order."""
    row, col, val, rm = _arrays(*_random(3000, 30, seed=5))
    monkeypatch.setenv("XCK_WRITE_CHUNK_ENTRIES", "64"); monkeypatch.setenv("XCK_WRITE_THREADS", "4")
    if knob is None: monkeypatch.delenv("XCK_WRITE_MAP", raising=False)
    else: monkeypatch.setenv("XCK_WRITE_MAP", knob)
    assert _write(lib, "/dev/null", row, col, val, rm, 30, 77) == 0
    fifo = tmp_path / "pipe.mtx"
    os.mkfifo(fifo)
    got = []
    t = threading.Thread(target=lambda: got.append(open(fifo, "rb").read()))
    t.start()
    rc = _write(lib, fifo, row, col, val, rm, 30, 77)          # (ctypes releases the GIL for the call: the reader drains meanwhile)
    t.join(30)
    assert rc == 0 and not t.is_alive()
    assert got[0] == _text(row, col, val, rm, 30, 77)


_CHILD = r"""
import ctypes as C, resource, signal, sys
import numpy as np
from xcltk_amd import capi
lib = capi.load()
n = 20000
row = np.sort(np.arange(n, dtype=np.int32) % 50); col = np.arange(n, dtype=np.int32); val = np.full(n, 123456, np.int32); rm = np.arange(1, 51, dtype=np.int32)
coo = capi.Coo(); coo.nnz = n
P = C.POINTER(C.c_int32)
coo.row = row.ctypes.data_as(P); coo.col = col.ctypes.data_as(P); coo.val = val.ctypes.data_as(P)
signal.signal(signal.SIGXFSZ, signal.SIG_IGN)
resource.setrlimit(resource.RLIMIT_FSIZE, (65536, 65536))       # the text is ~ 300 kB
rc = lib.xck_write_mtx(sys.argv[1].encode(), C.byref(coo), rm.ctypes.data_as(P), 50, n)
print("rc", rc, flush=True)
"""


@pytest.mark.parametrize("knob", [None, "0", "1"])
def test_file_size_limit_is_an_error_code_not_a_signal(tmp_path, knob):
    """A child whose RLIMIT_FSIZE lies below the text's size (SIGXFSZ ignored): the allocation fails, so nothing is mapped that could
    raise SIGBUS in the fill; the pipeline, which takes over, meets the limit in pwrite.  XCK_E_IO, and the child exits normally."""
    env = dict(os.environ, PYTHONPATH=ROOT, XCK_WRITE_CHUNK_ENTRIES="1000", XCK_WRITE_THREADS="3")
    env.pop("XCK_WRITE_MAP", None)
    if knob is not None: env["XCK_WRITE_MAP"] = knob
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path / "limited.mtx")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stdout.strip() == "rc -4", r.stdout                # XCK_E_IO


def test_real_chunk_size(lib, tmp_path, monkeypatch):
    """About 3 M entries at the chunk size a run uses (twelve chunks, the last one partial), a fifth of the rows dropped."""
    n = 3_000_017
    rng = np.random.default_rng(11)
    row, col, val, rm = _arrays(np.sort(rng.integers(0, 20000, n)), rng.integers(0, 10000, n), rng.integers(1, 50000, n), np.zeros(20000))
    keep = rng.random(20000) < 0.8; rm[keep] = np.arange(1, int(keep.sum()) + 1)
    monkeypatch.delenv("XCK_WRITE_CHUNK_ENTRIES", raising=False); monkeypatch.setenv("XCK_WRITE_THREADS", "5")
    outs = []
    for knob in (None, "1"):
        if knob is None: monkeypatch.delenv("XCK_WRITE_MAP", raising=False)
        else: monkeypatch.setenv("XCK_WRITE_MAP", knob)
        fn = tmp_path / ("big%s.mtx" % (knob or ""))
        assert _write(lib, fn, row, col, val, rm, int(rm.max()), 10000) == 0
        outs.append(fn.read_bytes())
    assert outs[0] == outs[1]
    kept = rm[row] > 0
    lines = outs[0].split(b"\n")
    assert lines[2] == b"%d\t10000\t%d" % (int(rm.max()), int(kept.sum())) and len(lines) == 3 + int(kept.sum()) + 1
    first, last = (int(i) for i in np.flatnonzero(kept)[[0, -1]])
    assert lines[3] == b"%d\t%d\t%d" % (rm[row[first]], col[first] + 1, val[first]) and lines[-2] == b"%d\t%d\t%d" % (rm[row[last]], col[last] + 1, val[last])
