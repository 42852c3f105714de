"""bench.py's launcher logic on the CPU: `--gpus N` without a torchrun environment starts N CHILD rank processes
through torch.distributed.run on 127.0.0.1 (and never touches the GPU or replaces the process first); inside a
torchrun environment it must not spawn again; WORLD_SIZE and --gpus must agree."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gpus_n_spawns_child_ranks(monkeypatch):
    bench = load_bench()
    import subprocess
    seen = {}

    def fake_call(cmd, env=None, **kw):
        seen["cmd"], seen["env"] = list(cmd), dict(env)
        return 0
    monkeypatch.setattr(subprocess, "call", fake_call)
    monkeypatch.setattr(bench.torch.cuda, "device_count", lambda: 4)
    monkeypatch.setattr(bench.torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("GPU touched before spawning")))
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "3", "--no-cpu-baseline"])
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert exc.value.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nnodes=1" in cmd and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1"
    assert 0 < int(cmd[cmd.index("--master-port") + 1]) < 65536
    script = cmd.index(os.path.join(ROOT, "bench.py"))
    tail = cmd[script + 1:]
    assert tail[tail.index("--gpus") + 1] == "4" and tail[tail.index("--steps") + 1] == "7"
    assert tail[tail.index("--warmup") + 1] == "3" and "--no-cpu-baseline" in tail
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"


def test_more_gpus_than_visible_is_refused(monkeypatch):
    bench = load_bench()
    monkeypatch.setattr(bench.torch.cuda, "device_count", lambda: 1)
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert "only 1 GPU" in str(exc.value.code)


def test_world_size_must_match_gpus(monkeypatch):
    bench = load_bench()
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4"])
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert "WORLD_SIZE=2" in str(exc.value.code)


def test_dump_outputs_is_passed_to_the_ranks(monkeypatch, tmp_path):
    bench = load_bench()
    import subprocess
    seen = {}
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None, **kw: seen.setdefault("cmd", list(cmd)) and 0)
    monkeypatch.setattr(bench.torch.cuda, "device_count", lambda: 2)
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--dump-outputs", str(tmp_path / "out")])
    with pytest.raises(SystemExit):
        bench.main()
    tail = seen["cmd"][seen["cmd"].index(os.path.join(ROOT, "bench.py")) + 1:]
    assert tail[tail.index("--dump-outputs") + 1] == str(tmp_path / "out")


@pytest.mark.parametrize("full", [False, True])
def test_full_is_passed_to_the_ranks_only_when_asked(monkeypatch, full):
    bench = load_bench()
    import subprocess
    seen = {}
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None, **kw: seen.setdefault("cmd", list(cmd)) and 0)
    monkeypatch.setattr(bench.torch.cuda, "device_count", lambda: 2)
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"] + (["--full"] if full else []))
    with pytest.raises(SystemExit):
        bench.main()
    tail = seen["cmd"][seen["cmd"].index(os.path.join(ROOT, "bench.py")) + 1:]
    assert ("--full" in tail) == full


def test_zero_steps_is_refused(monkeypatch):
    bench = load_bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert exc.value.code == 2


def test_dump_outputs_writes_the_same_sample_every_time(tmp_path):
    """dump_outputs on CPU stand-ins of the estimator: float arrays only, a fixed sample of large outputs, whole small
    ones, per-layer norms over every entry, identical files for identical inputs, well under 64 MB."""
    import numpy as np
    import torch
    bench = load_bench()
    torch.manual_seed(0)
    layers = [torch.nn.Linear(700, 900), torch.nn.Conv2d(64, 96, 3, bias=False), torch.nn.Linear(1200, 10)]

    class Est:
        state = {l: [torch.randn(k, k), torch.randn(n, n)] for l, k, n in ((layers[0], 701, 900), (layers[1], 576, 96),
                                                                          (layers[2], 1201, 10))}
        inv_state = {l: (torch.randn_like(a), torch.randn_like(g)) for l, (a, g) in state.items()}
    owned = list(enumerate(layers))
    infos = [bench.dump_outputs(str(tmp_path / f"d{r}"), layers, Est, owned) for r in range(2)]
    assert infos[0]["bytes"] == infos[1]["bytes"] < 64 << 20
    names = ["factor_layers"] + [n + s for n in ("weights", "factor_A", "factor_G", "inverse_A", "inverse_G")
                                 for s in ("", "_norms")]
    assert sorted(infos[0]["arrays"]) == sorted(names)
    for name in names:
        a, b = (np.load(tmp_path / f"d{r}" / f"{name}.npy") for r in range(2))
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), name
    w = np.load(tmp_path / "d0" / "weights.npy")
    assert w.size == sum(p.numel() for l in layers for p in l.parameters())              # 0.9 M entries: all of them
    assert np.array_equal(w, torch.cat([p.detach().reshape(-1) for l in layers for p in (l.weight, l.bias)
                                        if p is not None]).numpy())
    fa = np.load(tmp_path / "d0" / "factor_A.npy")                                         # 2.1 M entries: a sample
    assert 0.7 * bench.DUMP_SAMPLE < fa.size <= bench.DUMP_SAMPLE               # distinct indices of 2^20 draws
    flat = torch.cat([Est.state[l][0].reshape(-1) for l in layers]).numpy()
    assert np.isin(fa, flat).all()
    norms = np.load(tmp_path / "d0" / "inverse_G_norms.npy")
    assert np.allclose(norms, [float(torch.linalg.norm(Est.inv_state[l][1].double())) for l in layers])
    assert np.array_equal(np.load(tmp_path / "d0" / "factor_layers.npy"), [0.0, 1.0, 2.0])
