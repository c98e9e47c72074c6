"""bench.py starts its own ranks: `python bench.py --gpus N` with no launcher environment spawns N processes through
torch.distributed.run (before anything touches a GPU), relays rank 0's JSON line and the job's exit code
(the reference's multi-GPU run is one command too, README.md:34)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    return p.returncode, lines, p.stderr


def _torchrun(bench_args, env_extra=None, timeout=600, nproc=2):
    """The driver's form: `python -m torch.distributed.run --nproc-per-node N bench.py ...`, with every rank's stdout /
    stderr redirected to files of its own (--redirects 3 --tee 3 --log-dir), so that a failure is reported with the
    traceback of the rank that failed FIRST -- torchrun's own summary (all that `stderr[-3000:]` of the launcher shows) names
    the rank but cuts its traceback.  Returns (rc, JSON lines of the launcher's stdout, failure report)."""
    import glob
    import socket
    import tempfile
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    with tempfile.TemporaryDirectory(prefix="cgcn_launch_") as logs:
        p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc),
                            "--master-addr", "127.0.0.1", "--master-port", str(port), "--redirects", "3", "--tee", "3",
                            "--log-dir", logs, os.path.join(ROOT, "bench.py")] + bench_args,
                           env=env, capture_output=True, text=True, timeout=timeout)
        report = ""
        if p.returncode != 0:
            per_rank = []
            for f in sorted(glob.glob(os.path.join(logs, "**", "stderr.log"), recursive=True)):
                txt = open(f, errors="replace").read()
                first = txt.find("Traceback")
                per_rank.append((os.path.getmtime(f) if first >= 0 else float("inf"), f, txt[first:] if first >= 0 else txt[-1500:]))
            per_rank.sort(key=lambda t: t[0])
            report = "\n".join("==== %s ====\n%s" % (f[len(logs):], t[-4000:]) for _, f, t in per_rank)
            report += "\n==== launcher ====\n" + p.stderr[-1500:]
    # with --tee the ranks' stdout lines arrive prefixed "[default0]:"
    lines = [l[l.index("{"):] for l in p.stdout.splitlines() if "{" in l and l.lstrip().startswith(("{", "[default"))]
    lines = [l for l in lines if l.startswith('{"')]
    return p.returncode, lines, report


def test_self_launch_two_ranks_dry_run_prints_one_line():
    rc, lines, err = _run(["--gpus", "2", "--dry-run"])
    assert rc == 0, err[-2000:]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen_by_backend"] == 2 and d["dry_run"] is True


def test_self_launch_eight_ranks_dry_run_prints_one_line():
    """the driver's widest run: 8 ranks over the 16 train chromosomes (two step groups), one line from rank 0"""
    rc, lines, err = _run(["--gpus", "8", "--backend", "gloo", "--dry-run"], timeout=900)
    assert rc == 0, err[-2000:]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["ranks_seen_by_backend"] == 8 and d["dry_run"] is True


def test_single_rank_dry_run_needs_no_launcher():
    rc, lines, err = _run(["--dry-run"])
    assert rc == 0, err[-2000:]
    assert json.loads(lines[0])["n_gpus"] == 1


def test_plain_run_measures_the_headline_alone(monkeypatch):
    """a plain run sets up, warms up, times the steps and prints the line; roofline, CPU baseline and the secondary
    measurements run with --full only, where each keeps its own --no-* switch"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("cgcn_bench_cli", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    def parsed(*argv):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
        a = bench.parse()
        return a.full, a.no_extras, a.no_roofline, a.no_cpu_baseline
    assert parsed("--gpus", "1", "--steps", "3", "--warmup", "1") == (False, True, True, True)
    assert parsed("--full") == (True, False, False, False)
    assert parsed("--full", "--no-cpu-baseline") == (True, False, False, True)
    assert parsed("--full", "--no-extras", "--no-roofline") == (True, True, True, False)


def test_launcher_mismatch_is_an_error_not_an_assert():
    # under a launcher environment that disagrees with --gpus: refused with a message and a non-zero exit code
    rc, lines, err = _run(["--gpus", "4", "--dry-run"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert rc != 0 and not lines and "WORLD_SIZE=1" in err


def test_child_failure_is_relayed():
    # two ranks that cannot find a GPU (this test runs on the CPU tier) or, on a GPU box, are told to use more devices
    # than exist without --share-gpu: either way no JSON line and a non-zero exit code come back through the launcher
    rc, lines, err = _run(["--gpus", "64", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-extras"])
    assert rc != 0 and not lines


@pytest.mark.gpu
def test_self_launch_two_ranks_share_one_gpu_real_step():
    """the real engine behind the launcher: 2 ranks on one device (gloo: RCCL refuses two ranks per GPU), one
    chromosome per rank, gradient all-reduce + step"""
    rc, lines, err = _run(["--gpus", "2", "--backend", "gloo", "--share-gpu", "--workload", "chr21", "--steps", "3", "--warmup", "1",
                           "--no-cpu-baseline", "--no-extras", "--no-roofline"], timeout=900)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen_by_backend"] == 2 and d["value"] > 0 and d["scaling"] == "weak"


@pytest.mark.gpu
@pytest.mark.parametrize("gather", ["rank0", "all"])
def test_n_gt_1_code_path_over_rccl_with_one_forced_rank(gather):
    """bench.py's OWN multi-rank branch (process group with backend nccl = RCCL, deferred uploads, shard plan, the step
    group captured as one HIP graph with its all-reduce, prediction gather on the second communicator, max-over-ranks
    timing) on the one GPU a test box has: --force-collectives takes that branch with a one-rank group.  The loss after
    the same number of epochs must be the plain single-process run's up to the order of the optimizer steps (the shard
    plan walks the chromosomes largest first, the single process in the reference's order; a one-rank all-reduce is the
    identity)."""
    common = ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-extras", "--no-roofline"]
    rc, lines, err = _run(["--force-collectives", "--gather", gather] + common, timeout=900)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1
    d = json.loads(lines[0])
    c = d["config"]
    assert d["n_gpus"] == 1 and d["ranks_seen_by_backend"] == 1 and d["backend"] == "nccl"
    assert c["allreduce"] == "rccl" and c["step_group_graph"] is True and c["eager_collectives_on_own_communicator"] is True
    assert c["prediction_gather"].startswith(gather)
    rc1, lines1, err1 = _run(common, timeout=900)
    assert rc1 == 0, err1[-3000:]
    assert abs(json.loads(lines1[0])["final_loss"] - d["final_loss"]) < 2e-3 * abs(d["final_loss"])


@pytest.mark.gpu
def test_self_launch_eight_ranks_share_one_gpu_genome_epoch():
    """bench.py's own N = 8 branch on the real engine -- 8 processes on the one device (gloo), the 16 train
    chromosomes as two step groups of 8, rows of seven ranks gathered on rank 0 -- one JSON line, strong scaling"""
    rc, lines, err = _run(["--gpus", "8", "--backend", "gloo", "--share-gpu", "--steps", "2", "--warmup", "1",
                           "--no-cpu-baseline", "--no-extras", "--no-roofline"], timeout=1500)
    assert rc == 0, err[-3000:]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 8 and d["ranks_seen_by_backend"] == 8 and d["value"] > 0 and d["scaling"] == "strong"
    assert "rank0" in d["config"]["prediction_gather"]   # (gloo cannot send device tensors point to point: "all [asked for rank0: ...]")


# ---- the launch ladder: a rung that fails or hangs must cost a probe, not the run ---------------------
def test_ladder_first_rung_fails_second_runs():
    rc, lines, err = _run(["--gpus", "2", "--dry-run"], {"CGCN_BENCH_FAIL_RUNGS": "0"})
    assert rc == 0, err[-3000:]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    lad = d["launch_ladder"]
    assert lad["rung"] == 1 and d["rung"] == 1
    assert [t["ok"] for t in lad["tried"]] == [False, False, True] and "exit code" in lad["tried"][0]["why"]   # (a fast failure is retried once)
    assert lad["tried"][1].get("retry") is True and lad["tried"][1]["rung"] == 0
    # the measured job ran with the second rung's switches: eager all-reduce, predictions all-gathered
    assert d["no_group_graph"] is True and d["gather"] == "all" and d["hip_graph"] is True and d["probe"] is False


def test_ladder_hanging_probe_is_killed_and_the_next_rung_runs():
    rc, lines, err = _run(["--gpus", "2", "--dry-run"], {"CGCN_BENCH_HANG_RUNGS": "0,1", "CGCN_BENCH_PROBE_TIMEOUT_S": "20"}, timeout=300)
    assert rc == 0, err[-3000:]
    d = json.loads(lines[0])
    lad = d["launch_ladder"]
    assert lad["rung"] == 2 and [t["ok"] for t in lad["tried"]] == [False, False, True]
    assert "killed" in lad["tried"][0]["why"]
    assert d["no_group_graph"] is True and d["gather"] == "all" and d["hip_graph"] is False


def test_ladder_measured_job_failure_falls_through_to_the_next_rung():
    rc, lines, err = _run(["--gpus", "2", "--dry-run"], {"CGCN_BENCH_FAIL_MEASURED_RUNGS": "0"})
    assert rc == 0, err[-3000:]
    lad = json.loads(lines[0])["launch_ladder"]
    assert lad["rung"] == 1 and any(t.get("measured_job") and not t["ok"] for t in lad["tried"])


def test_ladder_every_rung_failing_is_an_error_with_the_history():
    rc, lines, err = _run(["--gpus", "2", "--dry-run"], {"CGCN_BENCH_FAIL_RUNGS": "0,1,2"})
    assert rc != 0 and not lines and "no rung of the launch ladder" in err


def test_external_launcher_probes_before_any_rank_touches_a_gpu():
    """the driver's form: `python -m torch.distributed.run ... bench.py --gpus N`.  Rank 0 probes with child jobs while
    the other ranks wait on the job's c10d store; every rank then runs with the chosen rung's switches."""
    rc, lines, report = _torchrun(["--gpus", "2", "--dry-run"], {"CGCN_BENCH_FAIL_RUNGS": "0"})
    assert rc == 0, report
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen_by_backend"] == 2
    lad = d["launch_ladder"]
    assert lad["rung"] == 1 and lad["launcher"].startswith("external")
    assert d["no_group_graph"] is True and d["gather"] == "all"


@pytest.mark.parametrize("late_rank", [0, 1])
def test_external_launcher_ranks_out_of_lockstep(late_rank):
    """round 4 initialised the default process group twice on the launcher's store (gloo meeting for the ladder,
    destroy, then the real group); whichever rank reached the second rendezvous first read its peer's stale address, so
    the run failed about half the time once the ranks were >= 1 s apart -- and passed whenever they were in lockstep,
    which is all the old test saw.  The skew is injected here: one rank sleeps 3 s between the ladder hand-off and the
    group's rendezvous; repeated CGCN_TEST_SKEW_REPEATS times per late rank (default 1: two runs in all; the old code failed 3 of 4 such runs; the
    fix was run 10 times in a loop by hand)."""
    for rep in range(int(os.environ.get("CGCN_TEST_SKEW_REPEATS", "1"))):
        rc, lines, report = _torchrun(["--gpus", "2", "--dry-run"],
                                      {"CGCN_BENCH_TEST_SKEW_RANK": str(late_rank), "CGCN_BENCH_TEST_SKEW_S": "3"})
        assert rc == 0, "repeat %d\n%s" % (rep, report)
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        assert d["ranks_seen_by_backend"] == 2 and d["launch_ladder"]["rung"] == 0


def test_hand_started_ranks_without_a_launcher_agent():
    """two ranks started by hand (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT in the environment, no torch.distributed.run,
    so no agent-hosted store): rank 0 hosts the job's c10d store itself, the ladder's choice and the process group go over it"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    base = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT",
                                                              "TORCHELASTIC_USE_AGENT_STORE", "TORCHELASTIC_RUN_ID")}
    procs = []
    for r in (1, 0):   # rank 1 first: it must wait for rank 0's store to come up
        env = dict(base, WORLD_SIZE="2", RANK=str(r), LOCAL_RANK=str(r), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   CGCN_BENCH_TEST_SKEW_RANK="0", CGCN_BENCH_TEST_SKEW_S="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry-run"], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=600) for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(o[1][-2000:] for o in outs)
    lines = [l for o in outs for l in o[0].splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["ranks_seen_by_backend"] == 2 and d["launch_ladder"]["rung"] == 0


def test_default_process_group_is_initialised_once_per_process():
    """the invariant behind the fix, checked on the source: bench.py reaches init_process_group through init_group only,
    and never destroys a group before the end of the job"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert src.count("dist.init_process_group(") == 1
    body = src[src.index("def external_ladder("):src.index("def _one_rank_allreduce(")]
    assert "dist.init_process_group(" not in body and "dist.destroy_process_group(" not in body and " init_group(" not in body


def test_failing_rank_traceback_is_reported():
    """a launcher-test failure must show the failing rank's own traceback, not torchrun's summary"""
    rc, lines, report = _torchrun(["--gpus", "2", "--dry-run", "--rung", "0"], {"CGCN_BENCH_FAIL_RUNGS": "0"})
    assert rc != 0 and not lines
    assert "rung 0 told to fail (test hook)" in report and "stderr.log" in report


def test_external_launcher_without_probes_runs_the_conservative_form():
    env = {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0", "CGCN_BENCH_LADDER": "0"}
    rc, lines, err = _run(["--gpus", "1", "--dry-run"], env)
    assert rc == 0, err[-2000:]
    assert "launch_ladder" not in json.loads(lines[0])   # one rank: nothing to choose


@pytest.mark.gpu
def test_external_launcher_on_the_gpu_box_probes_then_runs():
    """The driver's own form on real hardware: `python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2`, here
    with two gloo ranks sharing the one GPU a test box has.  Rank 0 must run the probe job(s) as children BEFORE either
    rank touches the GPU, both ranks must then run the measured job with the chosen switches, and the line must say so.
    One rank is held back 2 s before the group's rendezvous (the ranks of a real job are never in lockstep)."""
    rc, lines, report = _torchrun(["--gpus", "2", "--backend", "gloo", "--share-gpu", "--workload", "chr21", "--steps", "3",
                                   "--warmup", "1", "--no-cpu-baseline", "--no-extras", "--no-roofline"],
                                  {"CGCN_BENCH_TEST_SKEW_RANK": "0", "CGCN_BENCH_TEST_SKEW_S": "2"}, timeout=1200)
    assert rc == 0, report
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    lad = d["launch_ladder"]
    assert d["n_gpus"] == 2 and d["ranks_seen_by_backend"] == 2 and d["value"] > 0
    # (rung 0 on a healthy box; a transient start-up failure of a probe is retried, a second one moves the job to the next
    # rung -- the run is then still a success, which is the point of the ladder)
    assert lad["launcher"].startswith("external") and lad["rung"] in (0, 1, 2) and lad["tried"][-1]["ok"] is True
