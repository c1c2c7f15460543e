"""
bench.py's command line on the GPU: a plain run times the headline only and
says so in its one JSON line, --steps sets the number of timed steps, and
--dump-outputs writes the last timed step's trajectory entries and the engine
state after it -- the same arrays from run to run.  23 steps of 20-slice
episodes end on the slice graph, 40 on the episode graph.
"""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("features", "actions", "log_probs", "rewards", "state_q", "state_img", "state_ang")


def _bench(args):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def first_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump_a")
    line = _bench(["--gpus", "1", "--steps", "23", "--warmup", "3", "--dump-outputs", str(out)])
    return line, out


def test_plain_run_is_the_headline_alone(first_run):
    line, out = first_run
    assert line["steps"] == 23 and line["warmup"] == 3 and line["n_gpus"] == 1
    assert line["unit"] == "agent-steps/s" and line["higher_is_better"] is True
    assert np.isfinite(line["value"]) and line["value"] > 0
    # value = colloids x steps / timed seconds, ms_per_step = timed ms / steps
    assert line["value"] * line["ms_per_step"] * 1e-3 == pytest.approx(4096, rel=1e-9)
    assert line["windows"]["checked"] == 23  # one window per timed slice, one env
    for k in ("batched", "c2", "c4", "c5", "c3train", "dims3", "dense2d", "cpu_baseline",
              "cpu_baseline_all_cores", "cpu_baseline_all_pairs_vision", "slice_timeline_us"):
        assert k not in line
    assert sorted(os.listdir(out)) == sorted(f"{n}.npy" for n in NAMES)
    shapes = {"features": (1, 4096, 3, 1), "actions": (1, 4096), "log_probs": (1, 4096),
              "rewards": (1, 4096), "state_q": (3, 4096), "state_img": (3, 4096),
              "state_ang": (4096,)}
    for n in NAMES:
        a = np.load(out / f"{n}.npy")
        assert a.dtype in (np.float32, np.float64) and a.shape == shapes[n], n
        assert np.isfinite(a).all(), n
    acts = np.load(out / "actions.npy")
    assert set(np.unique(acts)) <= {0.0, 1.0, 2.0, 3.0} and len(np.unique(acts)) > 1
    assert (np.load(out / "log_probs.npy") <= 0).all()
    assert (np.load(out / "rewards.npy") >= 0).all()  # the clipped gradient reward


@pytest.fixture(scope="module")
def episode_run(tmp_path_factory):
    out = tmp_path_factory.mktemp("dump_e")
    line = _bench(["--gpus", "1", "--steps", "40", "--warmup", "0", "--dump-outputs", str(out)])
    return line, out


def test_steps_sets_the_timed_steps(first_run, episode_run):
    """40 timed steps: two episode-graph replays, 40 windows, another state
    than after 3 + 23 steps."""
    line, out = episode_run
    assert line["steps"] == 40 and line["windows"]["checked"] == 40
    assert sorted(os.listdir(out)) == sorted(f"{n}.npy" for n in NAMES)
    assert not np.array_equal(np.load(out / "state_q.npy"),
                              np.load(first_run[1] / "state_q.npy"))


@pytest.mark.parametrize("steps,warmup", [(23, 3), (40, 0)], ids=["slice_graph", "episode_graph"])
def test_dumped_outputs_repeat_from_run_to_run(request, tmp_path, steps, warmup):
    a = request.getfixturevalue("first_run" if steps == 23 else "episode_run")[1]
    b = tmp_path / "b"
    _bench(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs",
            str(b)])
    for n in NAMES:
        assert np.array_equal(np.load(a / f"{n}.npy"), np.load(b / f"{n}.npy")), n
