"""The lock micro-benchmarks' load generators resident on the GPU (dint_amd/csrc/k_lock_client.hip, driver.GpuLockClient)
and their closed loop through a lock engine (replay.LockLoop).

  - the device request stream is bit-identical to the host client's (FasstClient / LcgTplClient), epoch by epoch, each
    closing its own loop through its own GPU lock engine;
  - the free-running loop (no host inspection) leaves the lock table the CPU oracle has after the host client's stream;
  - lock_fasst is pinned to the unmodified reference: the 24M-op trace of tests/golden/fasst_24m.json recorded from the
    device reproduces the reference server's request / reply / table hashes and the client's outcome counters."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from dint_amd import _lib, wire
from dint_amd.driver import FasstClient, GpuLockClient, LcgTplClient
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FIX = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "fasst_24m.json")))
FASST, TPL = wire.Workload.FASST, wire.Workload.TPL
_HIP = None


def _hip():
    """the HIP runtime this process runs on (torch's copy, which libdint.so shares): copies between raw device pointers"""
    global _HIP
    if _HIP is None:
        import torch  # noqa: F401
        path = next(ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln)
        L = C.CDLL(path)
        L.hipMemcpyAsync.restype = C.c_int
        L.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        L.hipMemcpy.restype = C.c_int
        L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _HIP = L
    return _HIP


def _d2d(dst, src, nbytes, stream):
    assert _hip().hipMemcpyAsync(dst, src, nbytes, 3, stream) == 0  # hipMemcpyDeviceToDevice


def _h2d(dst, a):
    """the bytes of a numpy array to a raw device pointer (blocking)"""
    a = np.ascontiguousarray(a)
    if a.nbytes:
        assert _hip().hipMemcpy(dst, a.ctypes.data, a.nbytes, 1) == 0  # hipMemcpyHostToDevice


def _engine(wl, n_slots):
    from dint_amd.engine import Engine

    return Engine(wl, n_slots=n_slots, device=0)


def _host_client(wl, W, key_space, theta):
    return (FasstClient if wl == FASST else LcgTplClient)(W, key_space, zipf_theta=theta)


def _gpu_client(wl, W, key_space, theta, fuse, monkeypatch):
    monkeypatch.setenv("DINT_LOCK_CLIENT_FUSE", str(fuse))  # read when the client is created
    return GpuLockClient(wl, W, key_space, zipf_theta=theta, device=0)


# a sampled matrix of {fasst, 2pl} x {uniform, Zipf 0.8, Zipf 0.99} x W x fuse: every value of every axis, W = 300,000 above
# the engine's pass_max (65,536), 70,001 not a multiple of the workgroup
CASES = [
    (FASST, None, 1, 1, 300), (FASST, 0.8, 4096, 0, 60), (FASST, 0.99, 70_001, 1, 24), (FASST, 0.8, 300_000, 0, 10),
    (FASST, 0.99, 4096, 1, 60), (FASST, None, 300_000, 1, 10),
    (TPL, 0.99, 1, 0, 300), (TPL, None, 4096, 1, 60), (TPL, 0.8, 70_001, 0, 24), (TPL, 0.99, 300_000, 1, 10),
    (TPL, 0.8, 4096, 0, 60), (TPL, None, 70_001, 1, 24),
]


@pytest.mark.parametrize("wl,theta,W,fuse,epochs", CASES,
                         ids=[f"{'fasst' if c[0] == FASST else '2pl'}-{c[1] or 'uniform'}-W{c[2]}-fuse{c[3]}" for c in CASES])
def test_device_stream_equals_host_stream(wl, theta, W, fuse, epochs, monkeypatch):
    import torch

    key_space = 1 << 20
    hc, he = _host_client(wl, W, key_space, theta), _engine(wl, key_space)
    gc, ge = _gpu_client(wl, W, key_space, theta, fuse, monkeypatch), _engine(wl, key_space)
    st = torch.cuda.Stream()
    xs = st.cuda_stream
    for e in range(epochs):
        want = hc.next()
        rep = he.submit(want)
        hc.consume(rep)
        gc.next(xs)
        got = gc.read_batch()
        assert got.tobytes() == want.tobytes(), (e, np.nonzero(got.view(np.uint8).reshape(W, -1) != want.view(np.uint8).reshape(W, -1))[0][:8])
        ge.submit_device(gc.batch_ptr, W, gc.batch_ptr, xs)
        assert gc.read_batch().tobytes() == rep.tobytes(), e  # the replies, in place
        gc.consume(xs)
    hs, gs = hc.stats(), gc.stats()
    assert gs == hs
    assert hs["protocol_errors"] == 0 and hs["requests"] == W * epochs and hs["committed"] > 0
    assert hs["rejects"] > 0 or W == 1  # (one worker alone is never refused)
    a, b = he.read_locks(), ge.read_locks()
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()


@pytest.mark.parametrize("wl", [FASST, TPL], ids=["fasst", "2pl"])
def test_free_running_loop_equals_the_oracle(wl, monkeypatch):
    from dint_amd.replay import LockLoop

    W, key_space, theta, n = 70_001, 1 << 18, 0.99, 40
    gc, eng = _gpu_client(wl, W, key_space, theta, 1, monkeypatch), _engine(wl, key_space)
    loop = LockLoop(eng, gc)
    loop.epochs(n)
    loop.sync()
    hc = _host_client(wl, W, key_space, theta)
    o = orc.FasstOracle(key_space) if wl == FASST else orc.TplOracle(key_space)
    for _ in range(n):
        hc.consume(o.replay(hc.next()))
    assert o.errors == 0
    assert gc.stats() == hc.stats()
    a, b = eng.read_locks()
    if wl == FASST:
        assert (a == o.locks).all() and (b == o.vers).all()
    else:
        assert (a == o.num_ex).all() and (b == o.num_sh).all()
    assert eng.stats()["requests"] == W * n


def test_gpu_client_refuses_calls_out_of_order():
    gc = GpuLockClient(TPL, 1000, 1 << 16, device=0)
    L = gc._L
    assert L.dint_lock_gclient_consume(gc._h, None) == -5  # consume without next: DINT_ESTATE
    gc.next()
    assert L.dint_lock_gclient_next(gc._h, None) == -5  # a second next before consume
    gc.consume()
    gc.next()
    gc.consume()
    assert L.dint_lock_gclient_consume(gc._h, None) == -5
    assert gc.stats()["epochs"] == 2
    assert L.dint_lock_gclient_next(None, None) == -1 and L.dint_lock_gclient_read_batch(gc._h, None) == -1


def _sha(b) -> str:
    return hashlib.sha256(b).hexdigest()


def _dump_bytes(lock, ver) -> bytes:
    """the reference harness's state dump (tests/test_fasst_24m.py)"""
    nz = np.nonzero(lock | ver)[0].astype("<u4")
    rows = np.stack([nz, lock[nz].astype("<u4"), ver[nz].astype("<u4")], axis=1)
    return np.array([len(nz)], "<u4").tobytes() + rows.tobytes()


@pytest.mark.parametrize("n_req", [2_097_152, FIX["n_requests"]], ids=["prefix", "full"])
@pytest.mark.parametrize("variant", ["zipf0.8", "uniform"])
def test_fasst_24m_from_the_device_matches_the_reference(variant, n_req, monkeypatch):
    """W = 4096 workers over 24M keys, the engine at 36M slots: 5,859 full epochs and a last one cut to 24,000,000 requests
    (submitted with the shorter count, not consumed), recorded on the device"""
    import torch

    v, W = FIX["variants"][variant], FIX["n_workers"]
    gc = _gpu_client(FASST, W, FIX["key_space"], v["zipf_theta"], 1, monkeypatch)
    eng = _engine(FASST, FIX["n_slots"])
    req = torch.empty(n_req * 9, dtype=torch.uint8, device="cuda")
    rep = torch.empty(n_req * 9, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    xs = st.cuda_stream
    off = 0
    while off < n_req:
        cnt = min(W, n_req - off)
        gc.next(xs)
        _d2d(req.data_ptr() + off * 9, gc.batch_ptr, cnt * 9, xs)
        eng.submit_device(gc.batch_ptr, cnt, gc.batch_ptr, xs)
        _d2d(rep.data_ptr() + off * 9, gc.batch_ptr, cnt * 9, xs)
        if cnt == W:
            gc.consume(xs)
        off += cnt
    st.synchronize()
    eng.sync()
    if n_req == FIX["n_requests"]:
        assert _sha(req.cpu().numpy().tobytes()) == v["req_sha256"], "the device clients took another path"
        assert _sha(rep.cpu().numpy().tobytes()) == v["rep_sha256"]
        s = gc.stats()
        assert {k: s[k] for k in v["client"]} == v["client"] and s["protocol_errors"] == 0
        lock, ver = eng.read_locks()
        assert _sha(_dump_bytes(lock, ver)) == v["dump_sha256"]
        types = np.bincount(np.frombuffer(rep.cpu().numpy().tobytes(), wire.FASST_MSG)["type"], minlength=9)
        assert {str(k): int(c) for k, c in enumerate(types) if c} == v["reply_types"]
    else:
        assert _sha(req.cpu().numpy().tobytes()) == v["req_prefix_sha256"][str(n_req)]
        assert _sha(rep.cpu().numpy().tobytes()) == v["rep_prefix_sha256"][str(n_req)]
        assert gc.stats()["protocol_errors"] == 0
