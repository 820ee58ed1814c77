"""bench.py's plain run and --dump-outputs at a small geometry: the plain run
times the requested steps and reports the headline fields only (every other
leg waits for --full), and the dump holds what the last timed step left a
caller: the model output, every parameter's gradient, the state_dict after the
update — float arrays, the same from run to run."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

B, N, EMB, STEPS = 4, 256, 64, 3
FULL_ONLY = ("roofline", "fp32_exact_mode", "fp32_split_mode", "edgeconv_fwd_bwd_ms", "posemb_edge_mlp",
             "net_attention", "torch_eager_gpu", "cpu_baseline")


def _bench(out_dir, extra=()):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", "1",
           "--batch", str(B), "--points", str(N), "--emb", str(EMB), "--dump-outputs", str(out_dir), *extra]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.timeout(300)
@pytest.mark.parametrize("extra", [(), ("--no-graph",)], ids=["hip_graph", "eager"])
def test_bench_plain_run_and_dump(tmp_path, extra):
    from models.dgcnn import DGCNN
    r = _bench(tmp_path / "a", extra)
    assert r["steps"] == STEPS and r["full"] is False and r["unit"] == "clouds/s" and r["higher_is_better"] is True
    assert r["launch"] == ("eager" if extra else "hip_graph") and r["dtype"] == "bf16"
    assert r["ms_per_step"] > 0 and abs(r["value"] - B / r["ms_per_step"] * 1e3) <= 1e-2 * r["value"]
    assert r["eager_launch_ms_per_step"] is None and r["autocast_eager_ms_per_step"] is None
    assert not [k for k in FULL_ONLY if k in r]
    model = DGCNN(types.SimpleNamespace(emb_dim=EMB, k=20, in_dims=3))
    want = {"output": (B, EMB, N)}
    want.update({"grad." + n: tuple(p.shape) for n, p in model.named_parameters()})
    want.update({"param." + n: tuple(t.shape) for n, t in model.state_dict().items()})
    got = {f[:-4]: np.load(tmp_path / "a" / f, allow_pickle=False) for f in sorted(os.listdir(tmp_path / "a"))}
    assert {n: a.shape for n, a in got.items()} == want
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in got.values())
    assert got["param.conv1.1.num_batches_tracked"] > STEPS   # warm-up and timed steps all trained the model
    assert all(np.abs(got["grad." + n]).max() > 0 for n, _ in model.named_parameters())
    # a second run with the same arguments: the same seeded inputs, and the
    # engine's kernels sum in a fixed order (no float atomics), so the same bits
    _bench(tmp_path / "b", extra)
    for n, a in got.items():
        b = np.load(tmp_path / "b" / (n + ".npy"), allow_pickle=False)
        print(n, float(np.abs(a.astype(np.float64) - b).max()))
        assert np.array_equal(a, b), n
