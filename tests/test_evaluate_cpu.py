"""evaluate_ddpm.py's likelihood half on the host: compute_test_losses aggregates like reference utils/eval_helpers.py:24-34, the
seed keyword reaches test_losses per batch, and the CLI parses."""
import os
import subprocess
import sys

import torch

from utils import compute_test_losses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Stub:
    """test_losses returning per-batch values that depend on the batch and the keywords"""

    def __init__(self):
        self.calls = []

    def test_losses(self, x, **kw):
        self.calls.append(kw)
        b = x.shape[0]
        s = float(x.sum()) + float(kw.get("seed", 0))
        return {"vlb": torch.arange(b, dtype=torch.float32) * 0.25 + s, "L_simple": torch.tensor(0.5 * s + 1.0)}


def _loader(n, b=3):
    return [(torch.full((b, 1, 2, 2), 0.1 * (g + 1)), torch.zeros(b)) for g in range(n)]


def test_compute_test_losses_matches_reference_aggregation():
    loader = _loader(4)
    model = _Stub()
    vlb, l_simple = compute_test_losses(model, loader, "cpu")
    ref = _Stub()
    outs = [ref.test_losses(x) for x, _ in loader]
    want_vlb = torch.stack([o["vlb"] for o in outs], dim=1).mean().cpu().numpy().item()
    want_ls = torch.stack([o["L_simple"] for o in outs], dim=0).mean().cpu().numpy().item()
    assert vlb == want_vlb and l_simple == want_ls
    assert isinstance(vlb, float) and isinstance(l_simple, float)
    assert model.calls == [{}] * 4                       # seed=None: the reference's call, no keywords


def test_compute_test_losses_seeds_batches_and_stops_early():
    model = _Stub()
    compute_test_losses(model, _loader(5), "cpu", seed=10, max_batches=3)
    assert model.calls == [{"seed": 10}, {"seed": 11}, {"seed": 12}]


def test_evaluate_ddpm_help_parses():
    script = os.path.join(ROOT, "downsampled-diffusion_amd", "evaluate_ddpm.py")
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "downsampled-diffusion_amd"))
    r = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--saved_model", "--fid_samples", "--batch_size", "--seed", "--max_batches", "--synthetic", "--json"):
        assert flag in r.stdout
