"""The line bench.py prints LAST must stay parseable by the driver: a few KB of strict JSON carrying the contract's keys,
`roofline` and `cpu_baseline` (round 5's 20 KB line fell outside the driver's record: BENCH_r05.json `parsed: null`).
Built here from canned detail records (the full objects earlier rounds printed, committed under profiles/)."""
import glob
import json
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

# full records: the objects round 5 printed as its line, and round 6's bench_detail.json files of complete runs (with the CPU legs)
CANNED = [f for f in sorted(glob.glob(os.path.join(ROOT, 'profiles', 'r05_[mnp]_bench.json')) + glob.glob(os.path.join(ROOT, 'profiles', 'r06_*bench_detail.json')))
          if all(k in json.load(open(f)) for k in ('cpu_baseline', 'zpconv_roofline', 'other_configs', 'config3_step'))]
CONTRACT = ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config')


def _strict(text):
    def bad(tok):
        raise ValueError('non-finite constant in the line: ' + tok)
    return json.loads(text, parse_constant=bad)


@pytest.mark.parametrize('path', CANNED, ids=os.path.basename)
def test_compact_line_is_short_strict_json_with_the_judged_objects(path):
    full = json.load(open(path))
    line = bench.compact_line(full)
    text = json.dumps(line, allow_nan=False)
    assert '\n' not in text and len(text) < 8000, len(text)
    assert len(text) <= bench.LINE_BUDGET, len(text)
    back = _strict(text)
    for k in CONTRACT:
        assert k in back, k
    assert back['value'] == pytest.approx(full['value'], rel=1e-5) and back['dtype'] == 'f32' and 'workload' in back['config']
    roof = back['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic', 'kernel', 'avg_launch_ms'):
        assert k in roof, k
    assert roof['frac'] == pytest.approx(roof['achieved'] / roof['peak'], rel=1e-4)
    cpu = back['cpu_baseline']
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in cpu, k
    assert back['zpconv_roofline']['frac'] == pytest.approx(full['zpconv_roofline']['frac'], rel=1e-5)
    assert sorted(back['other_configs'].values()) == pytest.approx(sorted(c['value'] for c in full['other_configs']), rel=1e-5)
    assert back['config3_step']['value'] == pytest.approx(full['config3_step']['value'], rel=1e-5)
    assert back['detail'] == 'bench_detail.json'


def test_non_finite_numbers_become_null_and_the_budget_drops_side_objects_first():
    full = json.load(open(CANNED[-1]))
    full['roofline']['traffic'] = float('nan')
    full['zpconv_roofline']['ms'] = float('inf')
    full['other_configs'] = [dict(c, name=c['name'] + ' ' + 'x' * 400) for c in full['other_configs']] * 3    # an oversized side leg
    line = bench.compact_line(bench._clean(full))
    text = json.dumps(line, allow_nan=False)
    back = _strict(text)
    assert back['roofline']['traffic'] is None and back['zpconv_roofline']['ms'] is None
    assert 'roofline' in back and 'cpu_baseline' in back and math.isfinite(back['value'])


def test_a_failed_cpu_probe_keeps_the_line():
    full = json.load(open(CANNED[-1]))
    full['cpu_baseline'] = {'value': None, 'unit': 'point-clouds/sec', 'cores': 0, 'kind': 'port', 'error': 'RuntimeError("probe died")'}
    full.pop('speedup_vs_cpu_baseline', None)
    back = _strict(json.dumps(bench.compact_line(full), allow_nan=False))
    assert back['cpu_baseline']['error'].startswith('RuntimeError') and back['value'] > 0


def test_emit_writes_the_detail_file_and_prints_one_line(tmp_path, monkeypatch, capsys):
    full = json.load(open(CANNED[-1]))
    monkeypatch.setattr(bench, 'ROOT', str(tmp_path))
    os.makedirs(tmp_path / 'gpurun_out')
    bench.emit(full)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and _strict(out[0])['value'] == pytest.approx(full['value'], rel=1e-5)
    for d in (tmp_path, tmp_path / 'gpurun_out'):
        detail = _strict(open(d / 'bench_detail.json').read())
        assert 'kernels' in detail and 'launch_shapes' in detail


def test_dump_outputs_writes_float32_arrays_of_a_fixed_sample(tmp_path):
    """`--dump-outputs DIR` (bench.dump_outputs) on CPU tensors shaped as the step's: float32 .npy files, the features at the
    seeded point sample, the trained model's parameters, gradients and running statistics, within the budget."""
    import torch
    torch.manual_seed(0)
    feats = torch.randn(2, 8, 40, 60, dtype=torch.float64)
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.BatchNorm1d(4))
    model(torch.randn(5, 3)).sum().backward()
    last = {'feats': feats, 'pooled': feats.mean(2), 'pose_R': torch.randn(2, 2, 60, 3, 3), 'pose_T': torch.randn(2, 2, 60, 3),
            'loss': torch.tensor(1.5)}
    sizes = bench.dump_outputs(str(tmp_path / 'out'), last, model)
    files = sorted(p.name for p in (tmp_path / 'out').iterdir())
    assert files == sorted(k + '.npy' for k in sizes)
    for k in ('feats_sample', 'feats_pooled', 'pose_R', 'pose_T', 'loss', 'param.0.weight', 'grad.0.weight', 'buffer.1.running_mean'):
        assert k in sizes, k
    arrays = {k: np.load(tmp_path / 'out' / (k + '.npy')) for k in sizes}
    assert all(a.dtype == np.float32 for a in arrays.values())
    pts = bench.feats_sample_points(40, 2 * 8 * 60 * 8)
    assert np.array_equal(pts, bench.feats_sample_points(40, 2 * 8 * 60 * 8)) and len(pts) == 16 and len(set(pts.tolist())) == 16
    np.testing.assert_array_equal(arrays['feats_sample'], feats[:, :, torch.from_numpy(pts)].float().numpy())
    np.testing.assert_array_equal(arrays['grad.0.weight'], model[0].weight.grad.numpy())
    assert sum(sizes.values()) <= bench.DUMP_BUDGET
    # a larger output is sampled down to the budget, never written whole
    assert len(bench.feats_sample_points(4096, bench.FEATS_SAMPLE_BUDGET // 3)) == 3


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_and_dumps_its_outputs(tmp_path):
    """A plain `bench.py` run (no --full) on a small shape: one JSON line with the contract's keys and exactly --steps timed steps,
    and --dump-outputs writes the last step's outputs as finite float32 arrays."""
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '3', '--warmup', '1', '--batch', '1', '--points', '512',
                          '--dump-outputs', str(tmp_path / 'dump')], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-3000:]
    line = _strict(out.stdout.strip().splitlines()[-1])
    for k in CONTRACT:
        assert k in line, k
    assert line['steps'] == 3 and line['dtype'] == 'f32' and line['higher_is_better'] is True and 'roofline' not in line
    assert line['value'] == pytest.approx(1e3 / line['ms_per_step'], rel=1e-4)
    arrays = {p.stem: np.load(p) for p in (tmp_path / 'dump').glob('*.npy')}
    assert arrays['feats_sample'].shape == (1, 512, 16, 60) and arrays['feats_pooled'].shape == (1, 512, 60)
    assert arrays['pose_R'].shape == (1, 2, 60, 3, 3) and 'loss' in arrays and 'grad.convs.2.basic_conv.W' in arrays
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
    assert not (tmp_path / 'bench_detail.json').exists()
