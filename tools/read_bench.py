#!/usr/bin/env python3
"""Throughput of the batched read by position (cly_read_device, include/clyread.h).

Builds data files in HBM with libclygen, takes every record's position from
one cly_scan_device, then times cly_read_device (the library's HIP events:
cly_read_result.read_ms) over --reps calls after --warmup calls, with values
and as the verify-only pass.  Beside it, from the same process on the same
device: cly_scan_device's rate over the same files (the in-order yardstick)
and a one-core host loop of cly_db_value's read (byte-wise table CRC + memcpy)
over a bounded sample (the floor).

One JSON line goes to stdout and to profiles/read_<shape>_<order>.json.

    python tools/read_bench.py --shape c2 --order shuffled
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DATA_FILE_SIZE = 256 << 20


def zipf_lengths(n, rng, s=1.1, nmax=65473):
    w = np.arange(1, nmax + 1, dtype=np.float64) ** (-s)
    cdf = np.cumsum(w)
    cdf /= cdf[-1]
    return (63 + np.searchsorted(cdf, rng.random(n)) + 1).astype(np.uint32)


def make_files(shape, nbytes, torch, seed=0x434C59):
    from couloydb_amd import _abi
    gen = _abi.load_gen_lib()
    rng = np.random.default_rng(seed)
    if shape == "c2":               # 256-B values -> 276-B records
        vl = np.full(nbytes // 276, 256, np.uint32)
        typ = None
    elif shape == "zipf":           # Zipf value sizes 64 B .. 64 KiB
        vl = zipf_lengths(int(nbytes / 300), rng)
        vl = vl[:int(np.searchsorted(np.cumsum(vl.astype(np.int64) + 20), nbytes))]
        typ = None
    else:                           # tiny: 19-30-B records, a quarter tombstones
        n = int(nbytes / 24.5)
        vl = rng.integers(0, 12, n).astype(np.uint32)
        typ = (rng.random(n) < 0.25).astype(np.uint8)
        vl[typ == 1] = 0
    n = len(vl)
    recs = np.zeros(n, dtype=_abi.GEN_DTYPE)
    recs["value_len"] = vl
    recs["key_index"] = np.arange(n, dtype=np.int64) % 1_000_000_000
    if typ is not None:
        recs["type"] = typ
    maxf = 4096
    fo = (ctypes.c_uint64 * maxf)()
    fl = (ctypes.c_uint64 * maxf)()
    nf = ctypes.c_uint32()
    total = gen.cly_gen_layout(recs.ctypes.data, n, DATA_FILE_SIZE, 4096, fo, fl, maxf, ctypes.byref(nf))
    d_buf = torch.empty(int(total) + 4096, dtype=torch.uint8, device="cuda")
    d_recs = torch.from_numpy(recs.view(np.uint8)).to("cuda")
    rc = gen.cly_gen_encode(ctypes.c_void_p(d_buf.data_ptr()), ctypes.c_void_p(d_recs.data_ptr()), n, seed)
    if rc != 0:
        raise RuntimeError("cly_gen_encode failed: %d" % rc)
    torch.cuda.synchronize()
    files = [(d_buf.data_ptr() + int(fo[i]), int(fl[i]), i) for i in range(nf.value)]
    return d_buf, files, [int(fo[i]) for i in range(nf.value)], n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--shape", default="c2", choices=["c2", "zipf", "tiny"])
    ap.add_argument("--order", default="file", choices=["file", "shuffled"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=200_000, help="positions of the one-core host loop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    torch.cuda.init()
    from couloydb_amd import Scanner, _abi, build_info

    d_buf, files, file_off, n_gen = make_files(args.shape, args.bytes, torch)
    nbytes = sum(f[1] for f in files)
    sc = Scanner(0)
    cap = n_gen + 1024
    d_tup = torch.empty(cap * 6, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    scan_ms = []
    for _ in range(args.warmup + 5):
        t0 = time.perf_counter()
        first, res, st, need = sc.scan_device(files, d_tup.data_ptr(), cap)
        scan_ms.append((st.total_ms, (time.perf_counter() - t0) * 1e3))
    scan_ms = scan_ms[args.warmup:]
    n = int(need)
    assert n == n_gen and all(r.status == 0 for r in res), (n, n_gen)

    # positions from the scan's tuples: offset = word 0, fid = low half of word 3
    t6 = d_tup[:n * 6].view(n, 6)
    d_pos = torch.stack([t6[:, 0], t6[:, 3] & 0xFFFFFFFF], dim=1).contiguous()
    if args.order == "shuffled":
        g = torch.Generator(device="cuda")
        g.manual_seed(1234)
        d_pos = d_pos[torch.randperm(n, device="cuda", generator=g)].contiguous()
    d_out = torch.empty(n * 6, dtype=torch.int64, device="cuda")
    d_status = torch.empty(n, dtype=torch.int32, device="cuda")
    d_voff = torch.empty(n + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc, rr = sc.read_device(files, d_pos.data_ptr(), n, d_out.data_ptr(), d_status.data_ptr(), d_voff.data_ptr(),
                            None, 0)
    assert rc == 0 and rr.n_rec == n, (rc, rr.n_rec, n)
    vbytes, rbytes = int(rr.value_bytes), int(rr.record_bytes)
    d_val = torch.empty(vbytes + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def timed(values):
        ms = []
        for k in range(args.warmup + args.reps):
            rc, r = sc.read_device(files, d_pos.data_ptr(), n, d_out.data_ptr(), d_status.data_ptr(),
                                   d_voff.data_ptr(), d_val.data_ptr() if values else None, vbytes if values else 0)
            assert rc == 0 and r.n_rec == n
            if k >= args.warmup:
                ms.append(r.read_ms)
        return ms
    full = timed(True)
    verify = timed(False)

    # spot check of the gathered values: the first and last records against the file bytes
    tup = d_out.cpu().numpy().view(_abi.TUPLE_DTYPE)
    voff = d_voff.cpu().numpy()
    ok = True
    for i in (0, 1, n // 2, n - 1):
        t = tup[i]
        a = file_off[int(t["fid"])] + int(t["offset"]) + int(t["size"]) - int(t["value_size"])
        ok &= bool((d_buf[a:a + int(t["value_size"])] == d_val[int(voff[i]):int(voff[i + 1])]).all().item())

    # the floor: cly_db_value's loop on one core over a sample of file 0's positions
    lib = sc.lib
    lib.cly_dbg_read_host.restype = ctypes.c_uint64
    lib.cly_dbg_read_host.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                      ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_uint64)]
    h_file = d_buf[file_off[0]:file_off[0] + files[0][1]].cpu().numpy()
    pos_all = d_pos.cpu().numpy().view(np.int64).reshape(-1, 2)
    sel = pos_all[pos_all[:, 1] == 0][:args.host_sample]
    hp = np.zeros(len(sel), _abi.POS_DTYPE)
    hp["offset"] = sel[:, 0]
    hv = np.zeros(int(h_file.size), np.uint8)
    hvb, hrb = ctypes.c_uint64(), ctypes.c_uint64()
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        hn = lib.cly_dbg_read_host(h_file.ctypes.data, h_file.size, hp.ctypes.data, len(hp), hv.ctypes.data, hv.size,
                                   ctypes.byref(hvb), ctypes.byref(hrb))
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert hn == len(hp)

    def rate(ms_list, nb):
        m = statistics.median(ms_list)
        return {"ms_median": round(m, 4), "ms_min": round(min(ms_list), 4), "ms_max": round(max(ms_list), 4),
                "records_per_s": round(n / (m * 1e-3)), "GiB_per_s": round(nb / (m * 1e-3) / 2**30, 2)}
    scan_dev = statistics.median(x[0] for x in scan_ms)
    out = {
        "tool": "read_bench", "build": build_info(), "device": torch.cuda.get_device_name(0),
        "shape": args.shape, "order": args.order, "file_bytes": nbytes, "files": len(files), "records": n,
        "value_bytes": vbytes, "record_bytes": rbytes, "reps": args.reps, "warmup": args.warmup,
        "timer": "HIP events inside cly_read_device (read_ms); rates count record_bytes + value_bytes for the "
                 "read and record_bytes for verify-only",
        "read": rate(full, rbytes + vbytes),
        "verify_only": rate(verify, rbytes),
        "scan_device": {"ms_median": round(scan_dev, 4), "GiB_per_s": round(nbytes / (scan_dev * 1e-3) / 2**30, 2),
                        "records_per_s": round(n / (scan_dev * 1e-3))},
        "host_loop_one_core": {"positions": int(len(hp)), "s": round(best, 4),
                               "records_per_s": round(len(hp) / best),
                               "GiB_per_s": round((hrb.value + hvb.value) / best / 2**30, 3)},
        "values_spot_check": ok,
    }
    out["device_vs_host_loop"] = round(out["read"]["records_per_s"] / out["host_loop_one_core"]["records_per_s"], 1)
    line = json.dumps(out)
    print(line)
    path = args.out or os.path.join(ROOT, "profiles", "read_%s_%s.json" % (args.shape, args.order))
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "w") as f:
        f.write(line + "\n")
    sc.close()


if __name__ == "__main__":
    main()
