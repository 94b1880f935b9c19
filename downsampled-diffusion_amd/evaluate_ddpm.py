#!/usr/bin/env python3
"""Evaluation driver with the reference's behaviour (reference evaluate_ddpm.py:1-106), likelihood half: load
``{saved_model}.pt`` from CHECKPOINT_DIR (EMA weights preferred), rebuild the model from the stored config, run
``compute_test_losses`` over the test loader and print the reference's JSON metrics block.

The reference hard-codes its constants; here they are the defaults of optional flags.  The sample metrics (FID, sFID,
IS, precision / recall) need the TF-Inception evaluator, which is out of scope: their keys are
printed as null.  Extensions:
  * ``--seed S`` runs the native likelihood sweep (in-kernel Philox draws, batch g keyed by S + g; one C call per batch,
    graph-replayed steps); without it the reference's per-step loop with torch's generator runs;
  * ``--max_batches N`` stops after N test batches; ``--json OUT`` also writes the metrics to a file;
  * ``--synthetic CONFIG`` builds deterministic synthetic weights when no checkpoint exists (offline boxes);
  * ``--sample_acts S.npz --ref_acts R.npz`` (both or neither): Inception activations of the samples and of the reference set,
    computed elsewhere; the five sample-metric keys are then filled from them (utils/sample_metrics.py), null only where a file
    lacks the input a metric needs;
  * ``--kid`` (with ``--kid_subsets``, ``--kid_subset_size``) and ``--density_coverage``, with the activation files: the keys
    ``kid_mean`` / ``kid_std`` / ``kid_full`` and ``density`` / ``coverage`` follow the seven above (utils/sample_metrics.py
    extended_sample_metrics).  Without these flags the output is what it was.
"""
import argparse
import json
import time

import torch

from utils import DATA_DIR, compute_test_losses, get_dataloader
from utils.sample_metrics import extended_sample_metrics, sample_metrics
from utils.sampling_cli import load_model

SAMPLE_METRICS = ('is', 'fid', 'sfid', 'precision', 'recall')


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Test-set likelihood (VLB, L_simple) of a trained DDPM / dDDPM checkpoint.")
    ap.add_argument("--saved_model", default="celeba_x2")
    ap.add_argument("--fid_samples", type=int, default=50000, help="kept for the reference's interface (sample metrics are out of scope)")
    ap.add_argument("--batch_size", type=int, default=None, help="test batch size (default: the checkpoint's)")
    ap.add_argument("--seed", type=int, default=None, help="native sweep with Philox draws, batch g keyed by seed + g")
    ap.add_argument("--max_batches", type=int, default=None, help="stop after this many test batches")
    ap.add_argument("--synthetic", default=None, help="JSON config file: use closed-form synthetic weights, no checkpoint")
    ap.add_argument("--json", default=None, help="also write the metrics to this file")
    ap.add_argument("--sample_acts", default=None, help=".npz of the samples' Inception activations (pool_3, spatial, softmax)")
    ap.add_argument("--ref_acts", default=None, help=".npz of the reference set's activations, or its mu / sigma / mu_s / sigma_s")
    ap.add_argument("--kid", action="store_true", help="also report KID (kid_mean, kid_std over subsets; kid_full over all rows)")
    ap.add_argument("--kid_subsets", type=int, default=100, help="number of KID subsets")
    ap.add_argument("--kid_subset_size", type=int, default=1000, help="rows per KID subset (clamped to the smaller set)")
    ap.add_argument("--density_coverage", action="store_true", help="also report density and coverage (Naeem et al. 2020, k = 5)")
    args = ap.parse_args(argv)
    if (args.sample_acts is None) != (args.ref_acts is None):
        ap.error("--sample_acts and --ref_acts go together")
    if (args.kid or args.density_coverage) and args.sample_acts is None:
        ap.error("--kid and --density_coverage need --sample_acts and --ref_acts")
    if args.kid_subsets < 1 or args.kid_subset_size < 2:
        ap.error("--kid_subsets must be at least 1 and --kid_subset_size at least 2")
    return args


def main():
    args = parse_args()
    device = 'cuda'
    print(f'\nLoading model checkpoint {args.saved_model}')
    # (an old dDDPM config gets its force_latent, reference evaluate_ddpm.py:24-28; the batch size stays the checkpoint's unless given)
    model, config, _, step = load_model(args.saved_model, args.synthetic, args.batch_size, device, default_force_latent=True)
    print(f'Trained for {step} steps with configuration dict:')
    print(json.dumps(config, sort_keys=False, indent=4, default=str) + '\n')
    test_loader = get_dataloader(config, data_root=DATA_DIR, device=device, train=False)[0]

    ### COMPUTE METRICS ###
    print(f'\nComputing test losses over {args.max_batches if args.max_batches is not None else "all"} test batches')
    metrics = {}
    time_start = time.time()
    vlb, L_simple = compute_test_losses(model, test_loader, device, seed=args.seed, max_batches=args.max_batches)
    torch.cuda.synchronize()
    print(f'Test loss time: {time.time() - time_start}')
    metrics['vlb'] = vlb
    metrics['L_simple'] = L_simple
    if args.sample_acts is None:
        print('Sample metrics (IS, FID, sFID, precision, recall): the TF-Inception evaluator is out of scope; reported as null.')
        for k in SAMPLE_METRICS:
            metrics[k] = None
    else:
        print(f'Sample metrics from the activations {args.sample_acts} against {args.ref_acts}')
        time_start = time.time()
        if args.kid or args.density_coverage:
            scores = extended_sample_metrics(args.ref_acts, args.sample_acts, kid=args.kid, density_coverage=args.density_coverage,
                                             kid_subsets=args.kid_subsets, kid_subset_size=args.kid_subset_size)
        else:
            scores = sample_metrics(args.ref_acts, args.sample_acts)
        print(f'Sample metrics time: {time.time() - time_start}')
        for k in scores:                                    # the five SAMPLE_METRICS first, then the requested extensions
            metrics[k] = scores[k]

    # Display resulting metrics
    print('\nResults:')
    print(json.dumps(metrics, sort_keys=False, indent=4) + '\n')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(metrics, f, indent=4)


if __name__ == '__main__':
    main()
