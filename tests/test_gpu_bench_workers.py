"""bench.py's multi-process path with REAL workers and REAL kernels on the one GPU a test box has (the launcher had only ever run
--dry-run with more than one worker).  Both ways the driver may start it (BASELINE.json config 4):
  * `python bench.py --gpus 2` by itself with HIP_VISIBLE_DEVICES=0,0: the launcher narrows each child to "its" device (both are GPU 0 here),
    gloo barrier on 127.0.0.1;
  * under `python -m torch.distributed.run --nproc-per-node 2`: the worker asks for RCCL; two ranks on one GPU is something RCCL may refuse
    (duplicate device) -- then every rank must agree on gloo -- or serve; either way ONE well-formed line comes out.
Two ranks share the GPU, so the rates are not a scaling measurement; what is checked is that the sharded path runs kernels and reports.
Also here, from single-process runs: what --dump-outputs writes, and which entries a plain run and a --full one carry."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ['--gpus', '2', '--batch', '128', '--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--no-configs']


def clean_env(**extra):
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_ADDR', 'MASTER_PORT', 'TDS_BENCH_BACKEND', 'CUDA_VISIBLE_DEVICES'):
        e.pop(k, None)
    e.update(HSA_ENABLE_IPC_MODE_LEGACY='0', **extra)
    return e


def check(stdout, launcher_words):
    lines = [ln for ln in stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, stdout
    line = json.loads(lines[0])
    assert line['n_gpus'] == 2 and line['steps'] == 3 and line['warmup'] == 1 and line['scaling'] == 'weak'
    assert line['config']['global_batch'] == 256 and 'x2' in line['config']['parallelism'] and 'no collectives' in line['config']['parallelism']
    assert len(line['per_rank_agent_steps_per_s']) == 2 and all(v > 0 for v in line['per_rank_agent_steps_per_s'])
    assert line['value'] > 0 and 'dry_run' not in line and line['data'] == 'synthetic'
    # whole-job rate = all units / slowest rank's time: never above the sum of the per-rank rates
    assert line['value'] <= sum(line['per_rank_agent_steps_per_s']) * 1.0001
    roof = line['roofline']
    assert roof['kernel'] == 'raster_scene_bits_kernel' and roof['avg_launch_ms'] > 0 and 0 < roof['frac'] < 1      # kernels really ran
    assert any(w in line['launcher'] for w in launcher_words), line['launcher']
    assert [p['rank'] for p in line['per_rank']] == [0, 1] and all(p['avg_launch_ms'] > 0 and not p['ring_probe']['aliased'] for p in line['per_rank'])
    return line


def test_self_launch_two_real_workers_on_one_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *ARGS], capture_output=True, text=True, timeout=900,
                       env=clean_env(HIP_VISIBLE_DEVICES='0,0'))
    assert r.returncode == 0, r.stderr[-3000:]
    check(r.stdout, ['self-launch'])


def test_two_real_workers_under_torch_distributed_run():
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    r = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                        '--master-port', str(port), os.path.join(ROOT, 'bench.py'), *ARGS], capture_output=True, text=True, timeout=900,
                       env=clean_env(TDS_BENCH_RCCL_TIMEOUT='60'))
    assert r.returncode == 0, r.stderr[-3000:]
    line = check(r.stdout, ['external launcher'])
    assert 'RCCL barrier' in line['launcher'] or ('gloo' in line['launcher'] and 'falling back to gloo' in r.stderr)


def test_four_real_workers_on_one_gpu():
    """Many real workers sharing the one GPU of a test box: rendezvous of four children, four image rings probed side by side, four per-rank
    reports in the one line.  Four, not the eight of the driver's largest world (BASELINE.json config 4): a shared GPU takes
    at most six processes at once, and the test process already has it open."""
    args = ['--gpus', '4', '--batch', '64', '--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--no-configs', '--ring-candidates', '2']
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *args], capture_output=True, text=True, timeout=1500,
                       env=clean_env(HIP_VISIBLE_DEVICES='0,0,0,0'))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line['n_gpus'] == 4 and line['config']['global_batch'] == 256 and 'x4' in line['config']['parallelism']
    assert len(line['per_rank_agent_steps_per_s']) == 4 and all(v > 0 for v in line['per_rank_agent_steps_per_s'])
    assert line['value'] <= sum(line['per_rank_agent_steps_per_s']) * 1.0001
    per_rank = line['per_rank']
    assert [p['rank'] for p in per_rank] == list(range(4))
    for p in per_rank:
        assert p['avg_launch_ms'] > 0 and len(p['ring_probe']['kept']) == 2 and len(set(p['ring_probe']['kept'])) == 2 and not p['ring_probe']['aliased']
        assert len(p['ring_probe']['launch_ms']) >= 2 and p['ring_probe']['fill_ms'] > 0
    # the record says which physical GPU every rank sat on -- here all four on the one GPU of the box
    ids = [p['device_identity'] for p in per_rank]
    assert all(i['uuid'] not in (None, 'None') or i['pci'] for i in ids) and all(i['arch'].startswith('gfx950') and i['compute_units'] > 0 for i in ids)
    assert len({(i['uuid'], i['pci']) for i in ids}) == 1 and line['distinct_devices'] == 1
    assert all(i['reserved_usable'] in (True, False) for i in ids)


def test_plain_run_measures_the_headline_only_and_full_adds_the_rest():
    """A plain run sets up, warms up, times its steps and reports what those measured (the roofline from the timed launches, the image ring's
    probe); the entries that take runs of their own come with --full, and --no-default-path / --no-configs / --no-cpu-baseline still thin it"""
    base = ['--batch', '32', '--agents', '16', '--steps', '2', '--warmup', '1', '--ring-candidates', '2']
    extras = ('mixed_maps', 'default_path', 'roofline_u8', 'roofline_128', 'roofline_64', 'configs', 'cpu_baseline')
    same_run = ('measured_fill_gbs', 'measured_stream_gbs', 'measured_stream_ms')
    lines = []
    for more in ([], ['--full', '--no-configs', '--no-cpu-baseline']):
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), *base, *more], capture_output=True, text=True, timeout=900, env=clean_env())
        assert r.returncode == 0, r.stderr[-3000:]
        out = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(out) == 1, r.stdout
        lines.append(json.loads(out[0]))
    plain, full = lines
    for line in (plain, full):
        assert line['steps'] == 2 and line['warmup'] == 1 and line['value'] > 0 and line['ms_per_step'] > 0
        roof = line['roofline']
        assert roof['avg_launch_ms'] > 0 and roof['frac'] > 0 and roof['first_touch_ms'] > 0 and len(roof['ring_probe']['kept']) == 2
        assert roof['timed_raster_calls'][1] - roof['timed_raster_calls'][0] == 2
    assert plain['full'] is False and not any(k in plain for k in extras) and not any(k in plain['roofline'] for k in same_run)
    assert full['full'] is True and all(full['roofline'][k] > 0 for k in same_run)
    assert full['default_path']['ms_per_step'] > 0 and full['default_path']['avg_launch_ms'] > 0
    assert not any(k in full for k in extras if k != 'default_path')


def test_dump_outputs_are_the_last_timed_step(tmp_path):
    """--dump-outputs: what the timed loop computed in its LAST step (after --warmup + --steps steps), the same from run to run, within 64 MB;
    the state is the oracle's after that many steps of the seeded inputs, the metrics the oracle's on that state"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench
    from oracle import oracle as orc
    B, A, warmup, steps = 32, 16, 2, 3
    dumps = []
    for run in range(2):
        d = tmp_path / f'run{run}'
        r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--batch', str(B), '--agents', str(A), '--steps', str(steps), '--warmup', str(warmup),
                            '--no-cpu-baseline', '--no-configs', '--no-default-path', '--ring-candidates', '2', '--dump-outputs', str(d)],
                           capture_output=True, text=True, timeout=900, env=clean_env())
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.strip()][-1])
        assert line['steps'] == steps and line['warmup'] == warmup
        assert line['roofline']['timed_raster_calls'][1] - line['roofline']['timed_raster_calls'][0] == steps
        files = sorted(os.listdir(d))
        assert files == ['collision.npy', 'image_sums.npy', 'images.npy', 'offroad.npy', 'state.npy']
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        dumps.append({f[:-4]: np.load(d / f) for f in files})
    for k in dumps[0]:
        assert dumps[0][k].dtype in (np.float32, np.float64) and np.array_equal(dumps[0][k], dumps[1][k]), k
    out = dumps[0]
    assert out['state'].shape == (B, A, 4) and out['collision'].shape == out['offroad'].shape == (B, A)
    assert out['image_sums'].shape == (B, A, 3) and out['image_sums'].dtype == np.float64
    assert out['images'].shape == (bench.DUMP_IMAGES, 3, bench.RES, bench.RES)
    picked = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(B * A, bench.DUMP_IMAGES, replace=False))
    np.testing.assert_allclose(out['images'].sum((-2, -1), dtype=np.float64), out['image_sums'].reshape(B * A, 3)[picked], rtol=1e-9)
    verts, faces, vcat, cats = bench.load_town01()
    state, size, present, actions = bench.synth_agents(B, A, verts[vcat == cats.index('road')], 1234)
    for i in range(warmup + steps):
        state = orc.bicycle_step(state, actions[i % actions.shape[0]], np.full((B, A), 1.5, np.float32))
    np.testing.assert_allclose(out['state'], state, rtol=1e-5, atol=1e-4)
    s = out['state']
    sc = np.stack([np.sin(s[..., 2]), np.cos(s[..., 2])], -1).astype(np.float32)
    boxes = np.concatenate([s[..., :2], size, s[..., 2:3]], -1)
    np.testing.assert_allclose(out['collision'], orc.collision(boxes, present, metric='iou', sc=sc), rtol=0, atol=1e-5)
    np.testing.assert_allclose(out['offroad'], orc.offroad(s, size, verts, faces, 0.5, present=present, sc=sc), rtol=0, atol=1e-5)
