#!/usr/bin/env python3
"""Compare two datasets by their Inception activations, with the reference's behaviour (reference compare_datasets.py:1-47):
``ds_1`` acts as the reference batch, ``ds_2`` as the generative model; prints FID, sFID, precision and recall.

The reference reads two image arrays and runs the TF-Inception graph on them.  The network is out of scope here (SURVEY.md
section 2), so both arguments are ``.npz`` activation files written by any Inception port (utils/sample_metrics.py
load_activations: ``pool_3`` [N, 2048] and optionally ``spatial`` [N, 2023], or the ``mu`` / ``sigma`` / ``mu_s`` / ``sigma_s`` of a
published reference batch).  A metric whose input a file lacks is printed as null.  ``--json OUT`` also writes the metrics to a file.
``--kid`` (with ``--kid_subsets``, ``--kid_subset_size``) and ``--density_coverage`` append ``kid_mean`` / ``kid_std`` / ``kid_full`` and
``density`` / ``coverage`` (utils/sample_metrics.py extended_sample_metrics); without them the output is what it was.
"""
import argparse
import json

from utils.sample_metrics import EXTENDED_METRICS, extended_sample_metrics, load_activations, sample_metrics


def _min_max(acts):
    if acts.pool is None:
        return 'statistics only'
    return f'{acts.pool.min():.2f}\t{acts.pool.max():.2f}'


def main():
    ap = argparse.ArgumentParser(description="FID, sFID, precision and recall between two sets of Inception activations.")
    ap.add_argument("--ds_1", required=True, help=".npz activations (or statistics) of the reference batch")
    ap.add_argument("--ds_2", required=True, help=".npz activations of the generative model's samples")
    ap.add_argument("--json", default=None, help="also write the metrics to this file")
    ap.add_argument("--kid", action="store_true", help="also report KID (kid_mean, kid_std over subsets; kid_full over all rows)")
    ap.add_argument("--kid_subsets", type=int, default=100, help="number of KID subsets")
    ap.add_argument("--kid_subset_size", type=int, default=1000, help="rows per KID subset (clamped to the smaller set)")
    ap.add_argument("--density_coverage", action="store_true", help="also report density and coverage (Naeem et al. 2020, k = 5)")
    args = ap.parse_args()
    if args.kid_subsets < 1 or args.kid_subset_size < 2:
        ap.error("--kid_subsets must be at least 1 and --kid_subset_size at least 2")

    acts_1 = load_activations(args.ds_1)
    acts_2 = load_activations(args.ds_2)

    # print min-max values (of the pool_3 activations: the images themselves are not read here)
    print('\n\t\t\tMin\t\tMax')
    print(f'Dataset 1:\t{_min_max(acts_1)}')
    print(f'Dataset 2:\t{_min_max(acts_2)}')

    ### COMPUTE METRICS ###
    if args.kid or args.density_coverage:
        scores = extended_sample_metrics(acts_1, acts_2, kid=args.kid, density_coverage=args.density_coverage,
                                         kid_subsets=args.kid_subsets, kid_subset_size=args.kid_subset_size)
    else:
        scores = sample_metrics(acts_1, acts_2)
    metrics = {k: scores[k] for k in ('fid', 'sfid', 'precision', 'recall') + EXTENDED_METRICS if k in scores}

    # Display resulting metrics
    print('\nResults:')
    print(f'({args.ds_1} vs. {args.ds_2})')
    print(json.dumps(metrics, sort_keys=False, indent=4) + '\n')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(metrics, f, indent=4)


if __name__ == '__main__':
    main()
