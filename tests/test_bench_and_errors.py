"""bench.py's JSON contract and the ABI's error behaviour (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_bench_json_contract():
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "8", "--warmup", "2", "--config", "cfg2",
                          "--cpu-reps", "1", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly ONE JSON line"
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 8 and d["warmup"] == 2 and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and d["dtype"] == "int64" and d["data"] == "synthetic" and "workload" in d["config"]
    assert abs(d["value"] - d["config"]["logical_evals_per_step"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    r = d["roofline"]
    # the step is two latency-bound launches; HBM stays the nominal roofline the bytes are priced against
    assert r["bound"] == "latency" and r["nominal_bound"] == "hbm" and r["peak"] == 8000.0 and r["unit"] == "GB/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert abs(r["frac_per_eval_logical"] - d["value"] * r["bytes_per_eval"] / 8e12) < 1e-9 * r["frac_per_eval_logical"]
    # executed work at SURVEY 8(d)'s bytes — scan evals x (16 L + 2) + Filter evals x 65.125 — over the DOMINANT kernel's time
    wa, L = d["work_avoided"], 4
    exp_frac = (wa["prefilter_evals_executed"] * (16 * L + 2) + wa["filter_evals_executed"] * 65.125) / (r["avg_launch_us"] * 1e-6) / 8e12
    assert abs(r["frac_per_eval_executed"] - exp_frac) < 1e-6 * max(exp_frac, 1e-30) and r["frac_per_eval_executed"] <= 1.0
    rt = d["roofline_throughput"]                           # the real-work figure: launch B of the all-distinct step against its VALU issue bound
    assert rt["bound"] == "valu-issue" and 0.9 <= rt["k_compared_lanes"] <= 1.5 and rt["kernel_us"] > 0 and 0 < rt["frac"] <= 1.0
    assert abs(rt["frac"] - rt["evals_executed_per_launch"] / (rt["kernel_us"] * 1e-6) / rt["peak_evals_per_s"]) < 1e-9
    for k in ("k1", "k2", "k4"):                           # one utilisation figure per launch and k, each with the k the launch really compared
        e = rt["here"][k]
        assert 0 < e["frac"] <= 1.0 and e["k_compared_lanes"] > 0 and abs(e["peak_evals_per_s"] - 1024 * 2.4e9 / (rt["cycles_per_node_and_lane_at_the_bound"] * e["k_compared_lanes"]) * 64) < 1e-3 * e["peak_evals_per_s"]
    assert "issue_rate_frac" not in json.dumps(d)           # (round 5's second utilisation figure is gone: VERDICT r5 item 3)
    assert len(d["timed_regions_ms"]) >= 3 and abs(d["ms_per_step"] - d["timed_regions_ms"][0] / d["steps"]) < 1e-9
    assert abs(d["ms_per_step_median_region"] - float(np.median(d["timed_regions_ms"])) / d["steps"]) < 1e-9
    assert 0 < d["value_executed"] <= d["value"]
    assert "traffic" in r and "kernel" in r and r["avg_launch_us"] > 0
    for e in d["roofline_launches"]:                      # compulsory bytes / kernel-only time: nothing can exceed the roofline
        assert 0 < e["frac"] <= 1.0, e
        assert e["physical_frac"] is None or e["physical_frac"] <= 1.0
    if "rocprofv3 --kernel-trace" in r["time_source"]:     # every number in `roofline` is recomputable from kernel-only times
        assert r["sum_of_launch_us"] <= r["ms_per_step_us"] * 1.02, "the launches of a step cannot take longer than the step"
        assert r["kernel"] == max(d["roofline_launches"], key=lambda e: e["avg_launch_us"])["kernel"]
    assert d["value_resident"] == d["value"] and 10e6 < d["value_host_observed"] < d["value"]
    assert d["config"]["fast_path"] == 1 and d["config"]["launches_per_step"] == 2
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and "sample" in c and c["faithful_cost"] is False
    assert c["all_cores"]["cores"] >= 1 and c["all_cores"]["value"] > 0
    hc = d["host_cycle"]
    assert hc["gang_admit_latency_ms_p50"] <= hc["gang_admit_latency_ms_p95"] and hc["evals_per_s_at_p50"] > 10e6
    assert hc["modes"]["resident"]["rederives"] == 0 and hc["modes"]["resident"]["total"]["p50_ms"] <= hc["modes"]["latency"]["total"]["p50_ms"]
    dr = d["drain"]
    assert dr["gpu"]["gangs_released"] > 0 and dr["gpu"]["gang_admit_latency_ms_p50"] > 0 and dr["one_to_one_mode"]["prefilter_latency_ms_p50"] > 0
    assert c["sequential_pass"]["gangs_released"] > 0 and c["gang_admit_latency_ms_p50"] == c["sequential_pass"]["gang_admit_latency_ms_p50"]
    # the pod-by-pod pass on the device is the CPU pass, gang for gang; it is the headline gang-admit latency
    sd = dr["sequential_on_device"]
    assert sd["same_gangs_as_cpu_pass"] is True and sd["bit_identical_to_cpu_pass"] is True and dr["same_gangs_as_cpu_pass"] is True
    assert sd["gangs_released"] == c["sequential_pass"]["gangs_released"] and sd["pods_released"] == c["sequential_pass"]["pods_released"]
    assert d["gang_admit_latency_ms_p50"] == sd["gang_admit_latency_ms_p50"] > 0 and d["batched_cycle_latency_ms_p50"] == hc["gang_admit_latency_ms_p50"]
    assert set(d["scenarios"]) >= {"cold", "warm", "busy", "all_distinct_requests", "prefilter_only", "ms_per_step_by_seed"}
    fd = d["scenarios"]["filter_deny_on_device"]                # Filter's deny entry inside the batch: one more launch, a few microseconds
    assert fd["ms_per_step"] > 0 and fd["launches"] == d["config"]["launches_per_step"] + 1 and fd["pods_turned_away_by_filters_entry"] > 0
    assert d["value"] > 10e6, "north_star target: >= 10M pod x node fit evaluations/s"


def test_bench_plain_line_and_outputs(tmp_path, bsa, soa, orc):
    """A plain run (no --full): exactly --steps timed steps, a short line with the headline fields, and --dump-outputs writes what the
    timed path computed — equal to the oracle on the same seeded inputs."""
    dump = tmp_path / "out"
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "8", "--warmup", "2", "--config", "cfg2",
                          "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly ONE JSON line"
    assert len(lines[0]) < 4096, "a plain run's line stays short"
    d = json.loads(lines[0])
    assert d["metric"] == "pod x node fit evals/sec" and d["unit"] == "evals/s" and d["higher_is_better"] is True and d["dtype"] == "int64"
    assert d["steps"] == 8 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] - d["config"]["logical_evals_per_step"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    for key in ("roofline", "cpu_baseline", "host_cycle", "drain", "scenarios", "timed_regions_ms"):
        assert key not in d, f"{key} belongs to --full"
    nodes, fit, groups, pods, _ = bsa.synth.make("cfg2", "tail", seed=20260921)
    exp = orc.Sop(orc.Snapshot(nodes, fit), groups).batch(pods, soa.STAGE_ALL)
    got = {f[:-4]: np.load(dump / f) for f in os.listdir(dump)}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    for name in ("pf_code", "pf_first_k", "pf_leader", "fl_code", "fl_feasible", "group_admit", "group_ready"):
        assert np.array_equal(got[name], getattr(exp, name).astype(np.float64)), name
    idx = got["fl_bitmap_sample_pods"].astype(np.int64)
    assert len(idx) == min(pods.p, 512) and got["fl_bitmap_sample"].shape == (len(idx), nodes.n)
    node = np.arange(nodes.n)
    bits = (exp.fl_bitmap[node >> 6][:, idx] >> (node & 63).astype(np.uint64)[:, None]) & np.uint64(1)
    assert np.array_equal(got["fl_bitmap_sample"], bits.T.astype(np.float32))


def test_error_codes_not_crashes(bsa, soa):
    capi = bsa.capi
    nodes, fit, groups, pods, _ = bsa.synth.make("tiny", "warm")
    with bsa.Context(scalar_lanes=1) as ctx:
        with pytest.raises(capi.BsError) as e:
            ctx.run(soa.STAGE_ALL)                       # nothing loaded
        assert e.value.status == -4                      # BS_ERR_STATE
        ctx.load_nodes(nodes)
        with pytest.raises(capi.BsError):
            ctx.cluster_fits(0, 1.0, [0] * 5)            # fit masks not loaded
        ctx.load_fit(fit)
        with pytest.raises(capi.BsError) as e:
            ctx.cluster_fits(fit.n_classes, 1.0, [0] * 5)   # class out of range
        assert e.value.status == -1
        ctx.load_groups(groups)
        ctx.load_pods(pods)
        with pytest.raises(capi.BsError):
            ctx.run(soa.STAGE_FILTER)                    # PREFILTER is mandatory
        ctx.set_shard(0, 2)
        with pytest.raises(capi.BsError):
            ctx.run(soa.STAGE_ALL | soa.BATCH_COMMIT)    # COMMIT is single-rank only
        with pytest.raises(capi.BsError):
            ctx.set_shard(3, 2)
        ctx.set_shard(0, 1)
        out = ctx.batch(soa.STAGE_ALL)                   # still usable after the errors
        assert out.pf_code.shape == (pods.p,)
    with pytest.raises(capi.BsError):
        bsa.Context(scalar_lanes=13)                     # > BS_MAX_SCALARS
    with pytest.raises(capi.BsError):
        bsa.Context(scalar_lanes=0, device=99)           # no such device


def test_reference_panics_are_codes(bsa, soa, orc):
    """MinMember == 0 with Scheduled > 0 divides by zero in findMaxPG (core.go:716-717); Filter without a leader
    dereferences nil (core.go:525).  Both surface as codes."""
    import naive_ref as nv
    a, r = nv.Resource(), nv.Resource()
    a.Add({"cpu": 8000, "pods": 110})
    r.Add({"cpu": 0})
    info = nv.NodeInfo(a, r, 0)
    pg = nv.PodGroup("ns/z", 0, status_scheduled=2)
    pgs = nv.PGS(pg)
    pgs.pod = nv.Pod("rep", "ns/z", {"cpu": 100})
    cache = {"ns/z": pgs, "ns/y": nv.PGS(nv.PodGroup("ns/y", 3))}
    pods = [nv.Pod("u1", "ns/y", {"cpu": 100}), nv.Pod("u2", None, {"cpu": 100})]
    n, f, g, p, _ = nv.to_soa([info], cache, pods, [], 1)
    exp = orc.Sop(orc.Snapshot(n, f), g).batch(p, soa.STAGE_ALL)
    with bsa.Context(scalar_lanes=0) as ctx:
        ctx.load_nodes(n, f)
        ctx.load_groups(g)
        ctx.load_pods(p)
        got = ctx.batch(soa.STAGE_ALL)
    assert got.pf_code.tolist() == exp.pf_code.tolist() == [soa.PF_PANIC_DIV0, soa.PF_PASS_NOT_GROUPED]
    assert got.fl_code.tolist() == exp.fl_code.tolist()
