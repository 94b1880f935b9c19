#!/usr/bin/env python3
"""Compare two datasets by their Inception activations, with the reference's behaviour (reference compare_datasets.py:1-47):
``ds_1`` acts as the reference batch, ``ds_2`` as the generative model; prints FID, sFID, precision and recall.

The reference reads two image arrays and runs the TF-Inception graph on them.  The network is out of scope here (SURVEY.md
section 2), so both arguments are ``.npz`` activation files written by any Inception port (utils/sample_metrics.py
load_activations: ``pool_3`` [N, 2048] and optionally ``spatial`` [N, 2023], or the ``mu`` / ``sigma`` / ``mu_s`` / ``sigma_s`` of a
published reference batch).  A metric whose input a file lacks is printed as null.  ``--json OUT`` also writes the metrics to a file.
"""
import argparse
import json

from utils.sample_metrics import load_activations, sample_metrics


def _min_max(acts):
    if acts.pool is None:
        return 'statistics only'
    return f'{acts.pool.min():.2f}\t{acts.pool.max():.2f}'


def main():
    ap = argparse.ArgumentParser(description="FID, sFID, precision and recall between two sets of Inception activations.")
    ap.add_argument("--ds_1", required=True, help=".npz activations (or statistics) of the reference batch")
    ap.add_argument("--ds_2", required=True, help=".npz activations of the generative model's samples")
    ap.add_argument("--json", default=None, help="also write the metrics to this file")
    args = ap.parse_args()

    acts_1 = load_activations(args.ds_1)
    acts_2 = load_activations(args.ds_2)

    # print min-max values (of the pool_3 activations: the images themselves are not read here)
    print('\n\t\t\tMin\t\tMax')
    print(f'Dataset 1:\t{_min_max(acts_1)}')
    print(f'Dataset 2:\t{_min_max(acts_2)}')

    ### COMPUTE METRICS ###
    scores = sample_metrics(acts_1, acts_2)
    metrics = {k: scores[k] for k in ('fid', 'sfid', 'precision', 'recall')}

    # Display resulting metrics
    print('\nResults:')
    print(f'({args.ds_1} vs. {args.ds_2})')
    print(json.dumps(metrics, sort_keys=False, indent=4) + '\n')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(metrics, f, indent=4)


if __name__ == '__main__':
    main()
