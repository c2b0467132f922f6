"""CPU tests of bench.py's rank launcher (the driver's
`python bench.py --gpus N` runs): without an outer torch.distributed.run,
--gpus N starts N rank processes itself and rank 0's line reports n_gpus = N;
a WORLD_SIZE that disagrees with --gpus is an error.  --dry-protocol runs the
rank protocol (gloo barrier, MAX over ranks) with no GPU work.  Also the
--dump-outputs writer and, on a GPU, what a plain run prints and leaves out."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=240):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env,
                          cwd=ROOT)


def _lines(out):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("n", [2, 3])
def test_launcher_starts_n_ranks(n):
    r = _run(["--gpus", str(n), "--steps", "3", "--warmup", "1", "--dry-protocol"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _lines(r.stdout)
    assert len(lines) == 1, r.stdout
    line = lines[0]
    assert line["n_gpus"] == n and line["steps"] == 3 and line["warmup"] == 1
    pids = line["rank_pids"]
    assert len(pids) == n and len(set(pids)) == n
    # the launching process is none of the ranks
    assert all(isinstance(p, int) for p in pids)


def test_single_rank_runs_in_process():
    r = _run(["--gpus", "1", "--steps", "2", "--warmup", "0", "--dry-protocol"])
    assert r.returncode == 0, r.stderr[-2000:]
    (line,) = _lines(r.stdout)
    assert line["n_gpus"] == 1 and len(line["rank_pids"]) == 1


def test_world_size_mismatch_fails():
    r = _run(["--gpus", "4", "--dry-protocol"], env_extra={"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE" in r.stderr
    assert not _lines(r.stdout)



def test_dump_outputs_arrays(tmp_path, monkeypatch):
    """bench.dump_outputs over host tensors: float64 arrays, the tuple sample
    and the whole-output word sums equal the tuples' 32-bit words, the merged
    files' byte sample stays inside each file's length, and a second dump of
    the same data is identical (fixed sample seed)."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import bench

    class Res:
        def __init__(self, n, end, status):
            self.n_records, self.end_offset, self.status = n, end, status

    rng = np.random.default_rng(5)
    need = bench.DUMP_SAMPLE_TUPLES + 1000          # more tuples than the sample holds
    dfs = 4096
    monkeypatch.setattr(bench, "DATA_FILE_SIZE", dfs)
    lens = [4000, 4096, 100]
    wl = bench.Workload()
    wl.name = "c4"
    wl.d_out = torch.from_numpy(rng.integers(0, 256, (need + 8) * 48, dtype=np.uint8))
    wl.d_merge = torch.zeros(3 * dfs, dtype=torch.uint8)
    for k, ln in enumerate(lens):
        wl.d_merge[k * dfs:k * dfs + ln] = torch.from_numpy(rng.integers(1, 256, ln, dtype=np.uint8))
    wl.d_hint = torch.from_numpy(rng.integers(0, 256, 5000, dtype=np.uint8))
    mi = dict(out_lens=lens, hint_bytes=4500, n_live=7, n_reencoded=3, n_out_files=3)
    res = [Res(need - 5, 123456, 0), Res(5, 99, -3)]
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), 0, 1, torch, wl, [0, need - 5], res, need, mi)
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) < 64e6
    for name, a in got.items():
        assert np.array_equal(a, np.load(str(tmp_path / "b" / (name + ".npy")))), name
    words = wl.d_out[:need * 48].numpy().view(np.uint32).reshape(need, 12)
    idx = got["scan_tuple_index"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE_TUPLES and (np.diff(idx) > 0).all() and idx[-1] < need
    assert np.array_equal(got["scan_tuples"], words[idx])
    assert np.array_equal(got["scan_tuple_word_sums"][:, 0], (words & 0xFFFF).sum(0))
    assert np.array_equal(got["scan_tuple_word_sums"][:, 1], (words >> 16).sum(0))
    assert got["scan_needed"].tolist() == [need] and got["scan_status"].tolist() == [0, -3]
    assert got["scan_n_records"].tolist() == [need - 5, 5] and got["scan_end_offset"].tolist() == [123456, 99]
    pos = got["merge_byte_index"].astype(np.int64)
    assert len(pos) == sum(lens) and (pos % dfs < np.asarray(lens)[pos // dfs]).all()
    assert np.array_equal(got["merge_bytes"], wl.d_merge.numpy()[pos]) and (got["merge_bytes"] > 0).all()
    assert got["merge_file_byte_sums"].tolist() == [int(wl.d_merge[k * dfs:k * dfs + ln].sum()) for k, ln in enumerate(lens)]
    assert np.array_equal(got["hint_bytes"], wl.d_hint.numpy()[:4500]) and got["merge_out_lens"].tolist() == lens


@pytest.mark.gpu
def test_gpu_plain_run_is_lean_and_dumps(tmp_path):
    """A plain run (C1, the smallest configuration) prints the headline fields
    and none of the --full legs, honours --steps, and --dump-outputs writes
    the last step's results."""
    import numpy as np
    r = _run(["--gpus", "1", "--config", "c1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-2000:]
    (line,) = _lines(r.stdout)
    assert line["steps"] == 3 and line["warmup"] == 1 and line["parity_ok"] is True
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - line["config"]["bytes_per_gpu"] / (line["ms_per_step"] / 1e3) / 2**30) < 1e-2 * line["value"]
    for k in ("index", "append", "small_records", "host_path", "c5_n1", "index_load", "cpu_baseline"):
        assert k not in line, k
    assert "k_emit_ms" not in line["kernel"] and line["kernel"]["k_scan_ms"] > 0
    n = line["config"]["records_per_gpu"]
    assert np.load(str(tmp_path / "scan_needed.npy")).tolist() == [n]
    assert np.load(str(tmp_path / "scan_n_records.npy")).sum() == n
    t = np.load(str(tmp_path / "scan_tuples.npy"))
    assert t.dtype == np.float64 and t.shape == (n, 12)       # C1: fewer tuples than the sample size


def test_post_merge_open_merge_finished_record():
    """The post-merge open leg's merge-finished record (bench._record_bytes) is
    EncodeLogRecord of {MergeFinishedKey, strconv.Itoa(nonMergeFileId)}
    (merge.go:154-168), byte for byte the golden generator's encoding, and
    the oracle decodes it back."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    sys.path.insert(0, ROOT)
    import numpy as np

    import bench
    import make_golden as mg
    from oracle import cly_oracle as co
    for v in (b"0", b"128", b"4096", b"1000000"):
        rec = bench._record_bytes(mg.MERGE_FIN_KEY, v)
        assert rec == mg.encode_record(mg.MERGE_FIN_KEY, v)
        t, st, end = co.scan_file(np.frombuffer(rec, np.uint8).copy(), 0)
        assert len(t) == 1 and end == len(rec) and int(t["value_size"][0]) == len(v)
