#!/usr/bin/env python3
"""Sampling driver with the reference's behaviour (reference generate_model_samples.py:13-69): load
``{saved_model}.pt`` from CHECKPOINT_DIR (EMA weights preferred), rebuild the model from the stored config, draw
``fid_samples`` images in batches with ``model.sample``, convert with ``fix_samples`` and ``np.save`` the list of
batches (+ latent list for dDDPM), printing the same three timing lines.

The reference hard-codes its constants; here they are the defaults of optional flags.  Extensions:
  * runs one process per GPU under torchrun: rank 0 broadcasts the weights once (RCCL), every rank samples a contiguous
    run of the job's batches (no collective in the loop) and writes ``{saved_model}.rank{r}.npy``; rank 0 then merges the
    shards into the single ``{saved_model}.npy`` the evaluator loads (reference evaluate_ddpm.py:52).  A batch's draws
    (x_T, Philox key) depend only on its GLOBAL batch index, so the merged file is bit-identical to a 1-process run;
  * the device -> host stage is asynchronous (utils.OutputStage: pinned double buffer + events), so a batch's copy
    overlaps the next batch's sampling;
  * ``--synthetic CONFIG`` builds deterministic synthetic weights when no checkpoint exists (offline boxes);
  * ``--timestep_respacing SPEC``, ``--use_ddim`` and ``--eta`` (improved-diffusion's flag names) sample K of the T steps,
    ancestrally or with DDIM (models/diffusion/respace.py).  With any of them set the output name gains a suffix such as
    ``_ddim50_ddim_eta0``, so the full-chain samples of the same checkpoint are never overwritten;
  * ``--dpm_solver`` samples with DPM-Solver++(2M) over the ``--timestep_respacing`` steps (best on a log-SNR grid, e.g.
    ``logsnr20``); it excludes ``--use_ddim`` and ``--eta`` and writes e.g. ``{saved_model}_logsnr20_dpmpp2m.npy``.
"""
import argparse
import json
import os
import time

import numpy as np
import torch

from parallel import barrier, broadcast_module_, init_from_env, main_rank_does, shard_sizes
from utils import SAMPLE_DIR, SAMPLE_LATENT_DIR, OutputStage, merge_rank_shards
from utils import sampling_cli as cli


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="Generate samples from a trained DDPM / dDDPM checkpoint.")
    cli.add_chain_flags(ap, batch_size=192, solver=True, respacing_help='sample K of the T steps: "ddimN", "N" or "n1,n2,..." sections')
    ap.add_argument("--fid_samples", type=int, default=50000)
    ap.add_argument("--sample_every", type=int, default=1)
    ap.add_argument("--early_stop", type=int, default=None)
    ap.add_argument("--keep_shards", action="store_true", help="keep the per-rank .rank{r}.npy files after the merge")
    args = ap.parse_args(argv)
    cli.check_chain_flags(ap, args, "solver eta")
    return args


def main():
    args = parse_args()
    spaced = bool(args.timestep_respacing) or args.use_ddim or args.eta != 0.0 or args.dpm_solver
    sample_kw = cli.chain_kwargs(args) if spaced else {}
    # full-chain runs keep the reference's file names; spaced runs write beside them
    suffix = "_" + cli.chain_spec(args) if spaced else ""

    rank, world = init_from_env()
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if local >= torch.cuda.device_count():
        # several ranks on one GPU only work as a gloo rehearsal: RCCL wants one device per rank and would deadlock or error
        if world > 1 and torch.distributed.get_backend() != "gloo":
            raise RuntimeError(f"LOCAL_RANK {local} but only {torch.cuda.device_count()} GPU(s) visible: one process per GPU is "
                               "required with the nccl (RCCL) backend; set DDK_DIST_BACKEND=gloo to rehearse on one GPU")
        local = 0
    # ranks that share one GPU (the gloo rehearsal above, or a launcher that maps several ranks onto one device) cannot host a whole
    # cluster of the in-launch GroupNorm: switch that path off up front instead of waiting for its first (loud) give-up
    shared_gpu = world > 1 and (int(os.environ.get("LOCAL_RANK", "0")) >= torch.cuda.device_count()
                                or int(os.environ.get("LOCAL_WORLD_SIZE", "0")) > torch.cuda.device_count())
    if shared_gpu:
        print(f"[rank {rank}] several ranks share one GPU: the in-launch GroupNorm is switched off", flush=True)
    torch.cuda.set_device(local)
    device = f"cuda:{local}"

    # rank 0 fills the weights and broadcasts them once
    model, config, _, step = cli.load_model(args.saved_model, args.synthetic, args.batch_size, device, fill=rank == 0)
    broadcast_module_(model, src=0)
    if shared_gpu:
        model.latent_model.plan().set_option(model.latent_model.plan().OPT_CLUSTER_GROUPNORM, 0)

    # the job = ceil(fid_samples / batch) batches; rank r takes a contiguous run of them
    bs = config["batch_size"]
    n_batches_total = int(np.ceil(args.fid_samples / bs))
    mine = shard_sizes(n_batches_total, world)
    g0, n_batches = sum(mine[:rank]), mine[rank]
    if rank == 0:
        print(f"\nGenerating {args.fid_samples} samples from checkpoint {args.saved_model}.")
        print(f"Trained for {step} steps with configuration dict:")
        print(json.dumps(config, sort_keys=False, indent=4, default=str) + "\n")
    stage, latent_stage = OutputStage(), OutputStage()
    time_start = time.time()
    for g in range(g0, g0 + n_batches):
        torch.manual_seed(args.seed + g)          # x_T and the Philox key of batch g: the same on whichever rank runs it
        samples = model.sample(bs, args.sample_every, args.early_stop, **sample_kw)
        if config["model"] == "dddpm":
            samples, latent_samples = samples
            latent_stage.submit(latent_samples)
        stage.submit(samples)
    sample_list, latent_list = stage.finish(), latent_stage.finish()
    torch.cuda.synchronize()
    sampling_time = time.time() - time_start

    print(f"Using batch size {bs}")
    print(f"Total time: {sampling_time}")
    print(f"Sample time: {sampling_time / max(n_batches * bs, 1)}")
    print(f"Batch time: {sampling_time / max(n_batches, 1)}")

    def save(directory, name, batches):
        os.makedirs(directory, exist_ok=True)
        base = os.path.join(directory, name)
        if world == 1:
            np.save(base, batches, allow_pickle=False)
            return base
        # per-rank shards on a filesystem rank 0 can read (one node, or a shared mount: merge_rank_shards checks every shard exists)
        np.save(f"{base}.rank{rank}", batches, allow_pickle=False)
        barrier()                                   # every shard is on disk
        main_rank_does(lambda: merge_rank_shards(base, world, remove=not args.keep_shards) is None, "merge of the sampling shards")
        return base

    name = args.saved_model + suffix
    save_path = save(args.out_dir or SAMPLE_DIR, name, sample_list)
    if rank == 0:
        print(f"Samples saved to {save_path}")
    if config["model"] == "dddpm":
        save_path = save(args.out_dir or SAMPLE_LATENT_DIR, name + "_latent" if args.out_dir else name, latent_list)
        if rank == 0:
            print(f"Latent samples saved to {save_path}")


if __name__ == "__main__":
    main()
