"""bench.py's own multi-GPU launcher (BASELINE.json config 4), end to end on the CPU: `python bench.py --gpus 2 --dry-run`
starts one worker per rank, the workers rendezvous on 127.0.0.1 (gloo), run the barrier / timed loop / max-over-ranks path without
any kernel, and rank 0 prints ONE well-formed JSON line."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*argv, env=None):
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'TDS_BENCH_BACKEND'):
        e.pop(k, None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *argv], capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


# the self-launcher needs as many entries in the inherited device list as ranks: a box may export a list of one (HIP_VISIBLE_DEVICES=0)
TWO_DEVICES = dict(HIP_VISIBLE_DEVICES='0,1')


def check_line(line, n, steps, warmup):
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data',
              'config', 'roofline'):
        assert k in line, k
    assert line['n_gpus'] == n and line['steps'] == steps and line['warmup'] == warmup
    assert line['scaling'] == 'weak' and line['higher_is_better'] is True and line['unit'] == 'agent-steps/s'
    assert line['config']['global_batch'] == n * 1024 and line['config']['agents'] == 64
    assert f'x{n}' in line['config']['parallelism'] and 'no collectives' in line['config']['parallelism']
    assert line['value'] > 0 and line['dry_run'] is True
    # which device every rank ran on is part of the record (none in a dry run: no rank can tell, distinct_devices is null)
    assert 'distinct_devices' in line and line['distinct_devices'] is None
    reports = line['per_rank'] if n > 1 else [dict(device_identity=line['device_identity'])]
    for r in reports:
        assert set(r['device_identity']) >= {'device', 'uuid', 'pci', 'arch', 'compute_units', 'reserved_usable', 'visible'}


def test_self_launch_two_ranks_dry_run():
    line = check = run_bench('--gpus', '2', '--steps', '3', '--warmup', '1', '--dry-run', env=TWO_DEVICES)
    check_line(line, 2, 3, 1)
    assert len(line['per_rank_agent_steps_per_s']) == 2 and 'self-launch' in line['launcher']
    assert 'cpu_baseline' not in check                               # rank 0 of N = 1 only


def test_bad_arguments_are_refused():
    for argv, why in ((('--steps', '0', '--dry-run'), '--steps must be at least 1'),
                      (('--steps', '2', '--dry-run', '--dump-outputs', 'never_written'), 'a dry run computes nothing')):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *argv], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode != 0 and why in r.stderr, r.stderr
    assert not os.path.exists(os.path.join(ROOT, 'never_written'))


def test_device_list_is_narrowed_per_rank():
    # the launcher hands rank r the r-th entry of an inherited device list
    line = run_bench('--gpus', '2', '--steps', '1', '--warmup', '0', '--dry-run', env=dict(HIP_VISIBLE_DEVICES='5,3,1'))
    check_line(line, 2, 1, 0)
    assert [r['device_identity']['visible'] for r in line['per_rank']] == ['5', '3']


def test_distinct_devices_counts_physical_gpus():
    sys.path.insert(0, ROOT)
    import bench
    rep = lambda uuid, pci=None: dict(device_identity=dict(uuid=uuid, pci=pci))
    assert bench.distinct_devices([rep('a'), rep('b'), rep('a')]) == 2
    assert bench.distinct_devices([rep(None, '0000:05:00'), rep(None, '0000:05:00')]) == 1
    assert bench.distinct_devices([rep(None), rep('None')]) is None


def test_single_process_dry_run_and_torchrun_shape():
    line = run_bench('--steps', '2', '--warmup', '1', '--dry-run')
    check_line(line, 1, 2, 1)
    assert 'per_rank_agent_steps_per_s' not in line
    # the worker also runs under an external launcher that provides RANK / WORLD_SIZE (the driver's torch.distributed.run shape)
    line = run_bench('--gpus', '1', '--steps', '2', '--warmup', '1', '--dry-run', env=dict(RANK='0', LOCAL_RANK='0', WORLD_SIZE='1'))
    check_line(line, 1, 2, 1)


def test_the_line_says_whether_the_run_was_full():
    """a plain run and a --full one give the same headline fields; the line records which it was (the GPU side: tests/test_gpu_bench_workers.py)"""
    plain = run_bench('--steps', '2', '--warmup', '1', '--dry-run')
    full = run_bench('--steps', '2', '--warmup', '1', '--dry-run', '--full')
    for line in (plain, full):
        check_line(line, 1, 2, 1)
    assert plain['full'] is False and full['full'] is True
    line = run_bench('--gpus', '2', '--steps', '1', '--warmup', '0', '--dry-run', '--full', env=TWO_DEVICES)
    check_line(line, 2, 1, 0)
    assert line['full'] is True


def test_the_barrier_falls_back_to_gloo_when_rccl_cannot_come_up():
    """The process group only carries the barrier and the timing reductions.  Under an external launcher the worker asks for RCCL; where that
    fails both ranks must fall back to gloo and still deliver the line.  It fails here on every rank, GPU or not: the ranks name local devices
    that no box has (on a box with a GPU, one rank in a live RCCL rendezvous would wait for ever for a rank that failed)."""
    import socket
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(2):
        e = dict(os.environ, RANK=str(r), LOCAL_RANK=str(100 + r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), TDS_BENCH_DRY_RUN_TRY_NCCL='1')
        e.pop('TDS_BENCH_BACKEND', None)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--steps', '2', '--warmup', '1', '--dry-run'],
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=e))
    try:
        outs = [p.communicate(timeout=300) for p in procs]
    finally:
        for p in procs:                     # no rank outlives the test
            if p.poll() is None:
                p.kill()
                p.wait()
    assert all(p.returncode == 0 for p in procs), outs
    assert all('falling back to gloo' in err for _, err in outs), outs
    lines = [ln for ln in outs[0][0].splitlines() if ln.strip()]
    assert len(lines) == 1 and not outs[1][0].strip()
    line = json.loads(lines[0])
    check_line(line, 2, 2, 1)
    assert 'gloo' in line['launcher']


def test_traffic_figure_is_refused_for_another_build(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    val, note = bench.stamped_traffic(1024, 64)
    tj = json.load(open(os.path.join(ROOT, 'profiles', 'raster_traffic.json')))
    ent = tj.get('f32', tj)
    if ent.get('kernel_source_sha') == bench.kernel_source_stamp():
        assert val == ent['hbm_bytes_per_launch']
    else:
        assert val is None and 'refused' in note
    monkeypatch.setattr(bench, 'kernel_source_stamp', lambda: 'deadbeefdeadbeef')
    val, note = bench.stamped_traffic(1024, 64)
    assert val is None and 'refused' in note


def test_limiter_of_the_instruction_bound_modes_is_stamped_like_the_traffic(tmp_path, monkeypatch):
    """roofline_u8 / _128 / _64 say bound = 'valu' and quote the PMC-derived VALU figures of profiles/raster_traffic.json -- only for the build and the
    workload they were measured on"""
    sys.path.insert(0, ROOT)
    import bench
    fake = dict(u8=dict(batch=1024, agents=64, res=256, hbm_bytes_per_launch=1.3e10, kernel_source_sha='feedfacefeedface', source='profiles/x.json',
                        valu=dict(valu_busy_simds_per_se_of_32=29.3, valu_issue_fraction_of_add_chain=0.617, cycles_per_valu_instruction=6.5, valu_lane_occupancy=0.73, valu_instructions_per_launch=2.75e9, valu_issue_ms_at_4_cycles=4.48)),
                f32_64=dict(batch=1024, agents=64, res=64, hbm_bytes_per_launch=3.3e9, kernel_source_sha='feedfacefeedface', source='profiles/x.json', valu=None))
    monkeypatch.setattr(bench, 'ROOT', str(tmp_path))
    os.makedirs(tmp_path / 'profiles')
    json.dump(fake, open(tmp_path / 'profiles' / 'raster_traffic.json', 'w'))
    monkeypatch.setattr(bench, 'kernel_source_stamp', lambda: 'feedfacefeedface')
    lim = bench.stamped_limiter(1024, 64, 'u8')
    assert lim['bound'] == 'valu' and lim['valu_busy_simds_per_se_of_32'] == 29.3 and lim['cycles_per_valu_instruction'] == 6.5 and 'x.json' in lim['source']
    assert bench.stamped_limiter(256, 64, 'u8') == dict(bound='valu', note='PMC figure is for another workload')
    assert 'no PMC figure' in bench.stamped_limiter(1024, 64, 'f32_64', res=64)['note']          # an entry without VALU counters
    assert 'no PMC figure' in bench.stamped_limiter(1024, 64, 'f32_128', res=128)['note']
    monkeypatch.setattr(bench, 'kernel_source_stamp', lambda: 'deadbeefdeadbeef')
    lim = bench.stamped_limiter(1024, 64, 'u8')
    assert lim['bound'] == 'valu' and 'refused' in lim['note'] and 'valu_issue_fraction_of_add_chain' not in lim


def test_a_dying_worker_ends_the_launch_promptly():
    """rank 1 exits at start-up while rank 0 waits for it in the rendezvous: the launcher polls its children, reports the failure and
    ends rank 0 instead of waiting for the timeout"""
    import time
    t0 = time.time()
    e = dict(os.environ, TDS_BENCH_DRY_RUN_FAIL_RANK='1', **TWO_DEVICES)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'TDS_BENCH_BACKEND'):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--dry-run', '--steps', '2', '--warmup', '0'], capture_output=True,
                       text=True, timeout=300, env=e)
    assert r.returncode != 0 and 'worker 1 failed' in (r.stderr + r.stdout) and time.time() - t0 < 120
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith('{')]          # no result line from a failed launch


def test_dump_outputs_writes_float_arrays_within_the_budget(tmp_path, monkeypatch):
    """bench.dump_outputs on host tensors: every file float32 / float64; the per-camera arrays whole while they fit, a seeded sample of cameras
    once they would not (the GPU run: tests/test_gpu_bench_workers.py)"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    B, A = 8, 40
    g = torch.Generator().manual_seed(0)
    img = torch.rand(B, A, 3, 4, 4, generator=g) * 255
    state, col, off = torch.rand(B, A, 4, generator=g), torch.rand(B, A, generator=g), torch.rand(B, A, generator=g)
    sim = type('Sim', (), {'get_state': lambda self: state})()

    def dump(d):
        bench.dump_outputs(str(d), sim, img, col, off)
        return {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}

    out = dump(tmp_path / 'whole')
    assert sorted(out) == ['collision', 'image_sums', 'images', 'offroad', 'state']
    assert all(v.dtype in (np.float32, np.float64) for v in out.values()) and out['image_sums'].dtype == np.float64
    assert np.array_equal(out['state'], state.numpy()) and np.array_equal(out['collision'], col.numpy()) and np.array_equal(out['offroad'], off.numpy())
    np.testing.assert_allclose(out['image_sums'], img.double().sum((-2, -1)).numpy(), rtol=1e-12)
    picked = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(B * A, bench.DUMP_IMAGES, replace=False))
    assert np.array_equal(out['images'], img.reshape(B * A, 3, 4, 4).numpy()[picked])
    again = dump(tmp_path / 'again')
    assert all(np.array_equal(again[k], out[k]) for k in out)
    # a budget that holds the images and 100 cameras' worth of the rest
    monkeypatch.setattr(bench, 'DUMP_BYTES', out['images'].nbytes + 100 * (16 + 4 + 4 + 24))
    cut = dump(tmp_path / 'cut')
    assert sum(v.nbytes for v in cut.values()) <= bench.DUMP_BYTES
    assert cut['state'].shape == (100, 4) and cut['collision'].shape == cut['offroad'].shape == (100,) and cut['image_sums'].shape == (100, 3)
    rows = [int(np.flatnonzero((state.numpy().reshape(-1, 4) == r).all(1))[0]) for r in cut['state']]
    assert rows == sorted(rows) and np.array_equal(cut['collision'], col.numpy().reshape(-1)[rows])
    assert np.array_equal(cut['images'], out['images'])
