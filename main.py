#!/usr/bin/env python3
"""Drop-in CLI for the hot path of genome-minimizer-2's main.py (main.py:62-147, :647-692).

Implemented modes, same flags and file layout as the reference:
  --mode training --preset v0..v3 [--epochs N]     run_single_experiment (main.py:449-493)
  --mode sample --model-path ..._vK.pt --genes-path essential_gene_positions.pkl
        [--num-samples N] [--sampling-mode default|focused] [--noise-level s]   run_sampling (:219-446)
Both route through the gfx950 kernels of libgm2.so (gm2 package); there is no CPU path.

  --mode convert-samples --genes-path masks.npy [--output-file ids.npy]   run_binary_converter (:617-645)
        (host-side; the consumer of the sampled masks, explore_data/binary_converter.py)
  --mode minimizer --genes-path ids.npy [--genome-path wild_type.gb] [--single-file | --output-file f.fasta]
        [--output-dir d] [--model-name m]   run_genome_minimizer (:528-614), the consumer of the gene
        lists (gm2/minimizer.py: interval-union host rewrite of minimizer/minimizer_2.py)
Modes outside the MI355X hot path (explore, preprocess, experiment)
exit with code 2 and a message. Data files are looked up under the project root as in
utils/directories.py:13-20 (default: $GM2_PROJECT_ROOT or the current directory; --project-root).
Return codes follow main.py:647-692: 0 success, 1 failure.

Multi-GPU (no reference equivalent; the reference is single-device, main.py:37):
  python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 main.py --mode training ...
runs strain-row data parallelism over RCCL (gm2/ddp.py): every rank trains its share of each batch,
rank 0 prints and saves the checkpoint (--sync-bn: BatchNorm over the global batch, gm2/ddp.py).
--mode sample shards the genomes: one broadcast seed, the same z on every rank, each rank decodes its
contiguous slice on its GPU, rank 0 gathers the packed masks and writes the files. Other modes run
on rank 0 only.

Additions (no reference equivalent): --precision bf16|bf16x3|f32 for the training GEMMs (sampling always
decodes in exact fp32), --mask-dtype float64|uint8|bits for the saved masks (the reference writes
float64 via `.astype(float)`, main.py:369-371 / extras.py:200-201; uint8 keeps 1e6-genome runs in
memory; bits = numpy packbits(bitorder='little') rows, 1/64 of float64, accepted by convert-samples),
--no-csv to skip the genes x samples CSV. Sampling keeps the masks packed on the GPU: genome sizes
and essential-gene counts are computed there (gm2/masks.py) and only the packed rows cross PCIe.
--nearest-strains / --pca (sample mode, both off by default) compare the sampled genomes with the
dataset's strains on the packed rows (gm2_mask_nearest / gm2_mask_cooccur, gm2/pca.py): the nearest
strain of every sample by Hamming distance, and the PCA of the strains (the reference's Figure 2a)
with the samples projected onto its axes. --gene-frequencies (sample mode, off by default) counts the
genomes per gene of the sampled set and of the strains on the packed rows (gm2_mask_gene_counts,
gm2/genefreq.py) and writes the real-vs-sampled frequency table, per phylogroup for the strains and,
with --nearest-strains, for the samples by their nearest strain's phylogroup. --gene-linkage (sample
mode, off by default) compares which genes travel together: the gene x gene co-occurrence counts of a
panel of --linkage-genes intermediate-frequency genes in the strains and in the samples, from the
gene-major packed rows (gm2_mask_transpose, then gm2_mask_cooccur; gm2/linkage.py), as phi coefficients.
--minimized-sizes (sample mode, off by default; --genome-path, --minimized-fill essentials|none) reports
what convert-samples + --mode minimizer would make of every sampled genome -- genes removed, reduced
length, duplicate group -- from the packed rows and the GenBank record's gene features
(gm2_mask_minimized_stats; gm2/minsizes.py), without gene lists or FASTA.
--keep-smallest K (sample mode, off by default; --min-essential M, --search-chunk C) turns sampling into a
streaming search: --num-samples genomes are decoded chunk by chunk and only the K smallest distinct ones
that carry at least M essential genes (default: all of them) are kept, on the device (gm2_search_push;
gm2/search.py). The summary lines come from exact histograms over every genome screened; the winners'
masks, table and z are written, the consumers above run on the K winners, and no full-set file exists.
"""
import argparse
import os
import pickle
import sys
import traceback
from pathlib import Path

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "genome-minimizer-2_amd"))

MODES = ["training", "experiment", "minimizer", "explore", "preprocess", "sample", "convert-samples"]
IMPLEMENTED = ("training", "sample", "convert-samples", "minimizer")


def parse_arguments(argv=None):
    p = argparse.ArgumentParser(description="genome-minimizer-2 VAE hot path on MI355X")
    p.add_argument("--mode", choices=MODES, default="training")
    p.add_argument("--preset", choices=["v0", "v1", "v2", "v3"], default="v3")
    p.add_argument("--epochs", type=int, default=None)
    p.add_argument("--model-path", type=str)
    p.add_argument("--genes-path", type=str)
    p.add_argument("--output-file", type=str)
    p.add_argument("--num-samples", type=int, default=1)
    p.add_argument("--sampling-mode", choices=["default", "focused"], default="default")
    p.add_argument("--noise-level", type=float, default=0.1)
    p.add_argument("--project-root", type=str, default=os.environ.get("GM2_PROJECT_ROOT", os.getcwd()))
    p.add_argument("--precision", choices=["bf16", "bf16x3", "f32"], default="bf16")
    p.add_argument("--grad-exchange", choices=["f32", "bf16"], default=None,
                   help="torchrun / DDP only: dtype of the big weight-gradient all-reduce (default f32)")
    p.add_argument("--sync-bn", action="store_true",
                   help="torchrun / DDP only: train-mode BatchNorm over the global batch (SyncBN)")
    p.add_argument("--mask-dtype", choices=["float64", "uint8", "bits"], default="float64")
    p.add_argument("--no-csv", action="store_true")
    p.add_argument("--nearest-strains", action="store_true",
                   help="sample mode: Hamming distance of every sampled genome to its nearest dataset strain (CSV)")
    p.add_argument("--pca", action="store_true",
                   help="sample mode: PCA of the dataset strains with the sampled genomes projected onto it (CSV, PDF)")
    p.add_argument("--gene-frequencies", action="store_true",
                   help="sample mode: per-gene frequency of the sampled genomes against the dataset strains (CSV)")
    p.add_argument("--gene-linkage", action="store_true",
                   help="sample mode: gene-gene linkage (phi) of the sampled genomes against the dataset strains (CSV)")
    p.add_argument("--linkage-genes", type=int, default=2048,
                   help="sample mode, --gene-linkage: the most genes of the linkage panel")
    p.add_argument("--minimized-sizes", action="store_true",
                   help="sample mode: minimized genome size and duplicate group of every sampled genome (CSV), "
                        "computed on the packed masks without writing sequences")
    p.add_argument("--minimized-fill", choices=["essentials", "none"], default="essentials",
                   help="sample mode, --minimized-sizes: keep every essential gene as convert-samples' "
                        "_with_essentials lists do (essentials) or only the sampled genes (none)")
    p.add_argument("--keep-smallest", type=int, default=None, metavar="K",
                   help="sample mode: stream --num-samples genomes and keep only the K smallest distinct ones that "
                        "still have their essential genes (the full-set files are not written)")
    p.add_argument("--min-essential", type=int, default=None, metavar="M",
                   help="sample mode, --keep-smallest: essential genes a genome must carry (default: all of them)")
    p.add_argument("--search-chunk", type=int, default=65536, metavar="C",
                   help="sample mode, --keep-smallest: genomes decoded and screened per step")
    p.add_argument("--genome-path", type=str, default=None,
                   help="GenBank genome (default: <project root>/data/wild_type_sequence.gb)")
    p.add_argument("--output-dir", type=str, default="./minimized_genomes")
    p.add_argument("--single-file", action="store_true")
    p.add_argument("--model-name", type=str, default="default")
    return p.parse_args(argv)


def data_paths(root):
    """utils/directories.py:13-20."""
    d = os.path.join(root, "data")
    return {"Main Dataset": os.path.join(d, "F4_complete_presence_absence.csv"),
            "Phylogroups": os.path.join(d, "accessionID_phylogroup_BD.csv"),
            "Essential Genes": os.path.join(d, "essential_genes.csv")}


def check_data_availability(root):
    """main.py:149-170."""
    missing = [f"{k}: {v}" for k, v in data_paths(root).items() if not os.path.exists(v)]
    if missing:
        print("✗  Missing required data files:")
        for m in missing:
            print(f"   - {m}")
        return False
    print("✓ All required data files found")
    return True


PRECISION_NOTE = {
    "bf16": "bf16 GEMM operands, fp32 accumulation; fp32 master weights, BatchNorm, losses and Adam "
            "(--precision f32: the reference's fp32 arithmetic)",
    "bf16x3": "fp32 throughout, except the five gene-wide GEMMs of a step: fp32 operands split into bf16 hi + lo, "
              "hi.hi + hi.lo + lo.hi accumulated in fp32 (about 500x tighter than bf16; f32 is the reference's arithmetic)",
    "f32": "fp32 throughout (the reference's arithmetic)",
}


def _precision(args):
    from gm2 import native
    return {"f32": native.GM2_F32, "bf16x3": native.GM2_BF16X3}.get(args.precision, native.GM2_BF16)


def run_single_experiment(args):
    """main.py:449-493: preset config, optional epoch override, run the experiment."""
    from gm2.experiments import PRESETS, IntegratedExperimentRunner
    config = PRESETS[args.preset]()
    if args.epochs:
        config.n_epochs = args.epochs
    print(f"\n{'=' * 80}\nRunning {config.experiment_name} experiment")
    print(f"Hidden dim: {config.hidden_dim}, Latent dim: {config.latent_dim}")
    print(f"Epochs: {config.n_epochs}, Trainer: {config.trainer_version}")
    # (not in the reference's header: its arithmetic is fp32 throughout; this build's default is
    # bf16 GEMMs -- pass --precision f32 for the reference's arithmetic)
    print(f"Precision: {PRECISION_NOTE[args.precision]}\n{'=' * 80}")
    paths = data_paths(args.project_root)
    runner = IntegratedExperimentRunner(config, project_root=args.project_root, precision=_precision(args),
                                        dataset_csv=paths["Main Dataset"], phylogroups_csv=paths["Phylogroups"])
    results = runner.run_complete_experiment()
    print(f"\n{config.experiment_name.upper()} COMPLETED!")
    return results


def detect_version(model_path):
    """main.py:292-304: preset from the checkpoint file name."""
    name = Path(model_path).name.lower()
    for v in ("v0", "v1", "v2", "v3"):
        if v in name:
            return v
    return None


def focused_center(model, latent_dim, device):
    """main.py:351-366: 100 default samples, the one with fewest genes, then its output-space
    nearest sample's z (the same index) -> z* [1, L]."""
    import numpy as np
    from gm2.extras import sample_from_model
    binary_temp, cont_temp, z_temp = sample_from_model(model, latent_dim, 100, device)
    min_ones_index = np.argmin(binary_temp.sum(axis=1))
    dist = np.linalg.norm(cont_temp - cont_temp[min_ones_index], axis=1)
    closest = np.argmin(dist)
    return z_temp[closest].unsqueeze(0)


def focused_z(model, latent_dim, num_samples, noise_level, device):
    """main.py:351-370: the centre z* of focused_center, then z* + noise_level * N(0, I) [num_samples, L]."""
    import torch
    z_star = focused_center(model, latent_dim, device)
    noise = torch.randn(num_samples, latent_dim, device=device) * noise_level
    return z_star + noise


def focused_samples(model, latent_dim, num_samples, noise_level, device):
    """(u8 mask [N, G] on the device, z) of focused sampling."""
    z = focused_z(model, latent_dim, num_samples, noise_level, device)
    mask, _ = model.decode_mask(z)
    return mask, z


def gene_frequencies(packed, real, merged, nearest_idx, path):
    """--gene-frequencies: genomes per gene of the sampled set and of the strains, both counted on the
    packed rows (PackedMasks.gene_counts; no mask crosses PCIe for it), the strains also per phylogroup,
    the samples too when every sample has a nearest strain (--nearest-strains) whose phylogroup labels it."""
    import numpy as np
    from gm2 import genefreq
    groups = merged.iloc[:, -1].to_numpy()
    classes, by = real.gene_counts_by(groups)
    real_by = (classes, by, [int((groups == c).sum()) for c in classes])
    sampled_by = None
    if nearest_idx is not None:
        labels = groups[nearest_idx]
        s_classes, s_by = packed.gene_counts_by(labels)
        sampled_by = (s_classes, s_by, [int((labels == c).sum()) for c in s_classes])
    table = genefreq.frequency_table(merged.columns[:-1].to_numpy(), genefreq.gene_counts(real), real.n,
                                     genefreq.gene_counts(packed), packed.n, real_by, sampled_by)
    table.to_csv(path, index=False)
    s = genefreq.frequency_summary(table)
    print(f"- Gene frequencies, sampled vs real: Pearson r {s['pearson_r']:.4f}, |delta| mean {s['mean_abs_delta']:.4f}, "
          f"max {s['max_abs_delta']:.4f}")
    print(f"- Core genes of the strains (>= 99 %): {s['real_core']}; still core in the samples: "
          f"{s['real_core_sampled_core']}, at least soft core (>= 95 %): {s['real_core_sampled_soft_core']}")
    print(f"- Genes of the strains never sampled: {s['real_never_sampled']}; sampled but in no strain: "
          f"{s['sampled_absent_from_real']}\n- Gene frequencies: {path}")


def gene_linkage(packed, real, merged, k, path):
    """--gene-linkage: the panel (at most k genes of intermediate frequency in the strains), its gene x
    gene co-occurrence counts in the strains and in the samples (PackedMasks.gene_cooccurrence: both sets
    are transposed and counted on the device, no mask crosses PCIe for it), then the phi table."""
    from gm2 import genefreq, linkage
    panel = linkage.select_panel(genefreq.gene_counts(real), real.n, k=k)
    if len(panel) == 0:
        print("- Gene linkage: no gene of the strains has a frequency between 5 % and 95 %: nothing to compare")
        return
    both_real = real.gene_cooccurrence(panel).cpu().numpy()
    both_sampled = packed.gene_cooccurrence(panel).cpu().numpy()
    c_real, c_sampled = both_real.diagonal(), both_sampled.diagonal()
    table = linkage.linkage_table(merged.columns[:-1].to_numpy(), panel, both_real, c_real, real.n,
                                  both_sampled, c_sampled, packed.n)
    table.to_csv(path, index=False)
    s = linkage.linkage_summary(linkage.phi_matrix(both_real, c_real, real.n),
                                linkage.phi_matrix(both_sampled, c_sampled, packed.n))
    print(f"- Gene linkage, sampled vs real, {len(panel)} genes, {s['pairs']} pairs: Pearson r {s['pearson_r']:.4f}, "
          f"|delta phi| mean {s['mean_abs_delta']:.4f}, max {s['max_abs_delta']:.4f}")
    print(f"- Strongly linked pairs of the strains (|phi| >= 0.5): {s['real_strong']}; kept in the samples: "
          f"{s['real_strong_kept']}; strong in the samples only: {s['sampled_strong_new']}")
    print(f"- Panel genes constant in the samples: {s['sampled_constant']}\n- Gene linkage: {path}")


def compare_with_strains(args, packed, sizes, merged, out_dir, tag):
    """--nearest-strains / --pca / --gene-frequencies / --gene-linkage: the sampled genomes against the
    dataset's strains, on the device."""
    import numpy as np
    import pandas as pd
    from gm2.masks import PackedMasks
    real = PackedMasks.from_host(merged.iloc[:, :-1].to_numpy(), device=packed.bits.device)
    mode = args.sampling_mode
    idx = None
    if args.nearest_strains:
        ham, idx = packed.nearest(real)
        path = out_dir / f"{tag}_nearest_strain_{mode}.csv"
        pd.DataFrame({"sample": np.arange(packed.n), "nearest_strain": merged.index.to_numpy()[idx], "hamming": ham,
                      "genome_size": sizes}).to_csv(path, index=False)
        print(f"- Hamming distance to the nearest strain: median {np.median(ham):.0f}, range {ham.min()} - {ham.max()}")
        print(f"- Samples identical to a dataset strain: {int((ham == 0).sum())}\n- Nearest strains: {path}")
    if args.gene_frequencies:
        gene_frequencies(packed, real, merged, idx, out_dir / f"{tag}_gene_frequencies_{mode}.csv")
    if args.gene_linkage:
        gene_linkage(packed, real, merged, args.linkage_genes, out_dir / f"{tag}_gene_linkage_{mode}.csv")
    if args.pca:
        from gm2.pca import BinaryPCA
        pca = BinaryPCA(n_components=2)
        sc_real = pca.fit_transform(real)
        sc = np.concatenate([sc_real, pca.transform(packed)])
        path = out_dir / f"{tag}_pca_real_vs_sampled_{mode}.csv"
        source = np.array(["real"] * real.n + ["sampled"] * packed.n)
        pd.DataFrame({"PC1": sc[:, 0], "PC2": sc[:, 1], "source": source,
                      "phylogroup": list(merged["Phylogroup"].values) + [""] * packed.n}).to_csv(path, index=False)
        evr = pca.explained_variance_ratio_
        print(f"- PCA of the {real.n} strains: explained variance ratio PC1 {evr[0]:.4f}, PC2 {evr[1]:.4f}")
        print(f"- PCA scores (real and sampled): {path}")
        try:
            import matplotlib
            matplotlib.use("Agg")
            import matplotlib.pyplot as plt
        except ImportError:
            print("- matplotlib is not installed: no PCA scatter plot written")
            return
        fig, ax = plt.subplots(figsize=(7, 6))
        ax.scatter(sc[:real.n, 0], sc[:real.n, 1], s=6, alpha=0.5, label="real strains")
        ax.scatter(sc[real.n:, 0], sc[real.n:, 1], s=6, alpha=0.5, label="sampled genomes")
        ax.set_xlabel(f"PC1 ({100 * evr[0]:.1f} %)")
        ax.set_ylabel(f"PC2 ({100 * evr[1]:.1f} %)")
        ax.legend()
        fig.savefig(path.with_suffix(".pdf"))
        plt.close(fig)


def minimized_sizes(args, packed, sizes, path):
    """--minimized-sizes: what --mode convert-samples + --mode minimizer would report for these samples
    (reduced length, genes removed, duplicate groups), from the packed rows on the device
    (PackedMasks.minimized_stats, gm2/minsizes.py); no gene list and no FASTA is written."""
    import numpy as np
    import pandas as pd
    from gm2 import minsizes
    from gm2.minimizer import read_genbank
    genome_path = args.genome_path or os.path.join(args.project_root, "data", "wild_type_sequence.gb")
    if not os.path.exists(genome_path):
        print(f"✗ Genome file not found: {genome_path}")
        return False
    paths = data_paths(args.project_root)
    # the gene column names as run_binary_converter takes them
    large = pd.read_csv(paths["Main Dataset"], index_col=0)
    cols = large.drop(index=["Lineage"], errors="ignore").transpose().columns
    if len(cols) != packed.G:
        print(f"✗ The dataset has {len(cols)} gene columns, the sampled masks {packed.G}")
        return False
    essential_set = None
    if args.minimized_fill == "essentials":
        ess = pd.read_csv(paths["Essential Genes"])   # binary_converter.load_files
        essential_set = set(ess["# gene" if "# gene" in ess.columns else "gene"].astype(str).str.strip())
    plan = minsizes.FeaturePlan.build(read_genbank(genome_path), cols, essential_set)
    stats = packed.minimized_stats(plan)
    table = minsizes.size_table(stats, sizes, plan.L)
    table.to_csv(path, index=False)
    red, dup = stats["reduced_length"], minsizes.duplicate_stats(stats["signature"])
    print(f"- Minimized genomes ({Path(genome_path).name}, {plan.L:,} bp, {plan.F} gene features, "
          f"fill: {args.minimized_fill}): median reduced length {np.median(red):.0f} bp, "
          f"range {red.min()} - {red.max()}")
    print(f"- Mean reduction: {table['reduction_pct'].mean():.2f}%")
    print(f"- Unique minimized genomes: {dup['unique_sequences']} of {dup['total_sequences']}; "
          f"duplicate groups: {dup['duplicate_groups']}\n- Minimized sizes: {path}")
    return True


def run_smallest_search(args, model, config, merged, essential_gene_positions, out_dir, device):
    """--keep-smallest: --num-samples genomes streamed through gm2.search.search_smallest (its docstring
    is the draw order: per chunk one torch.randn, scaled around focused_center's z* in focused mode), then
    the K winners' summary, files and consumers. Under torchrun every rank streams its rank_slice with
    global indices and a generator seeded shared_seed + rank, and rank 0 merges the gathered states."""
    import numpy as np
    import pandas as pd
    import torch
    from gm2.ddp import get_dist, rank_slice, rank_world, shared_seed
    from gm2.search import SmallestSearch, hist_quantiles, search_smallest
    K, N, mode, tag = args.keep_smallest, args.num_samples, args.sampling_mode, config.trainer_version
    if K < 1 or K > 65536 or args.search_chunk < 1 or (args.min_essential is not None and args.min_essential < 0):
        print("✗ --keep-smallest takes 1..65536, --search-chunk >= 1, --min-essential >= 0")
        return False
    dist = get_dist()
    rank, world = rank_world(dist)
    generator = None
    if dist is not None:
        seed = shared_seed(dist)
        torch.cuda.manual_seed(seed)   # (the focused centre below: the same on every rank)
        generator = torch.Generator(device=device)
        generator.manual_seed(seed + rank)
    center = focused_center(model, config.latent_dim, device) if mode == "focused" else None
    lo, hi = rank_slice(N, rank, world)
    search = search_smallest(model, hi - lo, K, essential_gene_positions, args.min_essential, chunk=args.search_chunk,
                             z_center=center, noise_level=args.noise_level if center is not None else None,
                             generator=generator, base_index=lo, return_search=True)
    if dist is not None:
        mine = search.state_tensors()
        gathered = {}
        for name, t in mine.items():
            parts = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(parts, t.contiguous())
            gathered[name] = parts
        if rank != 0:
            return True
        for r in range(1, world):
            other = SmallestSearch(search.G, K, essential_gene_positions, args.min_essential,
                                   latent_dim=config.latent_dim, device=device, chunk_max=1)
            other.load_state_tensors({name: parts[r] for name, parts in gathered.items()},
                                     next_index=rank_slice(N, r, world)[1])
            search.merge(other)
    res = search.result()
    print(f"\n✓ Sampling Results:\n- Screened genomes: {res.seen}")
    q = hist_quantiles(res.size_hist)
    if q is not None:
        print(f"- Median genome size: {q[0]:.0f} genes\n- Genome size range: {q[1]:.0f} - {q[2]:.0f}")
        e = hist_quantiles(res.ess_hist)
        print(f"- Median essential genes: {e[0]:.0f}\n- Essential range: {e[1]:.0f} - {e[2]:.0f}")
    print(f"- Viable genomes (>= {search.min_groups} of {search.n_groups} essential genes): {res.viable} of {res.seen}")
    k = len(res.indices)
    if k:
        print(f"- Kept the {k} smallest distinct viable genomes: {res.sizes.min()} - {res.sizes.max()} genes")
    else:
        print("- No viable genome was found: nothing kept")
    packed = res.masks
    if k and (args.nearest_strains or args.pca or args.gene_frequencies or args.gene_linkage):
        compare_with_strains(args, packed, res.sizes, merged, out_dir, tag)
    if args.minimized_sizes and k and not minimized_sizes(args, packed, res.sizes,
                                                          out_dir / f"{tag}_minimized_sizes_{mode}.csv"):
        return False
    if args.mask_dtype == "bits":
        out = packed.to_host()
    else:
        out = packed.unpack(np.float64 if args.mask_dtype == "float64" else np.uint8)
    np.save(out_dir / f"{tag}_smallest_{mode}.npy", out)
    pd.DataFrame({"rank": np.arange(k), "sample": res.indices, "genome_size": res.sizes,
                  "essential_genes": res.essential}).to_csv(out_dir / f"{tag}_smallest_{mode}.csv", index=False)
    np.save(out_dir / f"{tag}_smallest_z_{mode}.npy", res.z.cpu().numpy())
    print(f"- Smallest genomes: {out_dir / f'{tag}_smallest_{mode}.csv'}")
    print(f"\n✓ SAMPLING COMPLETE!\n- Results saved to: {out_dir}")
    return True


def run_sampling(args):
    """main.py:219-446 without the reference's plots: load the checkpoint, decode in fp32, threshold,
    count essential genes, save masks (.npy) and the genes x samples CSV; --nearest-strains / --pca
    add the comparison with the dataset's strains (compare_with_strains)."""
    import numpy as np
    import torch
    from gm2.data import load_and_validate_data
    from gm2.experiments import PRESETS
    from gm2.extras import count_essential_genes, load_model, write_samples_to_dataframe

    if not args.model_path:
        print("✗ Model path required for sampling mode")
        return False
    if not os.path.exists(args.model_path):
        print(f"✗ Model file not found: {args.model_path}")
        return False
    if not args.genes_path or not os.path.exists(args.genes_path):
        print(f"✗ Model file not found: {args.genes_path}. Run preprocessing first.")
        return False
    paths = data_paths(args.project_root)
    _, merged, _ = load_and_validate_data(paths["Main Dataset"], paths["Phylogroups"])
    all_genes = merged.columns[:-1]
    input_dim = len(all_genes)
    print(f"Detected input dimension: {input_dim}")
    with open(args.genes_path, "rb") as f:
        # the user's own preprocessing output, read the way the reference reads it (main.py:273-274)
        essential_gene_positions = pickle.load(f)
    version = detect_version(args.model_path)
    if version is None:
        print("✗ Could not detect version")
        return False
    config = PRESETS[version]()
    out_dir = Path(args.project_root) / "models" / f"{version}_model" / "sampling_results"
    out_dir.mkdir(parents=True, exist_ok=True)
    device = torch.device("cuda", torch.cuda.current_device())
    model = load_model(input_dim, config.hidden_dim, config.latent_dim, args.model_path)
    print(f"- Architecture: {input_dim} -> {config.hidden_dim} -> {config.latent_dim}")
    print(f"- Samples: {args.num_samples}\n- Mode: {args.sampling_mode}\n- Output: {out_dir}")
    if args.keep_smallest is not None:
        return run_smallest_search(args, model, config, merged, essential_gene_positions, out_dir, device)
    from gm2.ddp import gather_rows, get_dist, rank_slice, rank_world, shared_seed
    dist = get_dist()
    rank, world = rank_world(dist)
    if dist is not None:
        # every rank draws the same z from one broadcast seed (the reference's z is one unseeded
        # draw of the global generator, extras.py:197) and decodes its contiguous slice
        torch.cuda.manual_seed(shared_seed(dist))
    if args.sampling_mode == "default":
        with torch.no_grad():
            z = torch.randn(args.num_samples, config.latent_dim, device=device)  # extras.py:197
    else:
        z = focused_z(model, config.latent_dim, args.num_samples, args.noise_level, device)
    lo, hi = rank_slice(args.num_samples, rank, world)
    st0 = model.decode_stats()
    packed, _ = model.decode_bits(z[lo:hi])   # masks stay on the GPU, 8 genes per byte
    st = {k: v - st0[k] for k, v in model.decode_stats().items()}
    # (this rank's decode: output-layer tiles per path and the certified band)
    print(f"- Decode (rank {rank}): {st['single_tiles']} bf16 / {st['split_tiles']} bf16x3 / {st['exact_tiles']} fp32 "
          f"output tiles; "
          f"{st['band_elements']} band logits recomputed in fp64, {st['band_flips']} bits changed"
          + (f"; {st['band_overflow']} past the list, their {st['overflow_tiles']} blocks recomputed whole in fp64"
             if st["band_overflow"] else ""))
    if dist is not None:
        # the ranks' packed slices -> the full set (rank 0 writes the reference's files)
        from gm2.masks import PackedMasks
        packed = PackedMasks(gather_rows(dist, packed.bits, args.num_samples), packed.G)
        if rank != 0:
            return True
    sizes = packed.row_sizes()                # binary.sum(axis=1)
    ess = count_essential_genes(packed, essential_gene_positions)  # on the device
    print(f"\n✓ Sampling Results:\n- Generated samples: {packed.n}")
    print(f"- Median genome size: {np.median(sizes):.0f} genes")
    print(f"- Genome size range: {np.min(sizes):.0f} - {np.max(sizes):.0f}")
    print(f"- Median essential genes: {np.median(ess):.0f}")
    print(f"- Essential range: {np.min(ess):.0f} - {np.max(ess):.0f}")
    if args.nearest_strains or args.pca or args.gene_frequencies or args.gene_linkage:
        compare_with_strains(args, packed, sizes, merged, out_dir, config.trainer_version)
    if args.minimized_sizes and packed.n and not minimized_sizes(
            args, packed, sizes, out_dir / f"{config.trainer_version}_minimized_sizes_{args.sampling_mode}.csv"):
        return False
    if args.mask_dtype == "bits":
        out = packed.to_host()
    else:
        out = packed.unpack(np.float64 if args.mask_dtype == "float64" else np.uint8)
    np.save(out_dir / f"{config.trainer_version}_binary_samples_{args.sampling_mode}.npy", out)
    if not args.no_csv:
        rows = out if args.mask_dtype != "bits" else packed.unpack(np.uint8)
        write_samples_to_dataframe(rows, all_genes, f"{out_dir}/{config.trainer_version}_data_full_samples_df.csv")
    print(f"\n✓ SAMPLING COMPLETE!\n- Results saved to: {out_dir}")
    return True


def run_binary_converter(args):
    """main.py:617-645: gene columns from the dataset CSV, masks -> gene-id lists, then the
    essential-gene fill (explore_data/binary_converter.py)."""
    import pandas as pd
    from gm2.binary_converter import check_essential_genes, load_files, masks_to_gene_lists
    if not args.genes_path:
        print("✗ --genes-path is required in convert-samples mode (input masks .npy)")
        return False
    if not os.path.exists(args.genes_path):
        print(f"✗ Input masks file not found: {args.genes_path}")
        return False
    out_path = args.output_file or "seq_out.npy"
    paths = data_paths(args.project_root)
    large = pd.read_csv(paths["Main Dataset"], index_col=0)
    cols = large.drop(index=["Lineage"], errors="ignore").transpose().columns
    masks_to_gene_lists(masks_npy_path=args.genes_path, cols=cols, out_ids_npy=out_path)
    essential_set, id_lists = load_files(paths["Essential Genes"], out_path)
    filled = check_essential_genes(essential_set, id_lists, out_path)
    print(f"✓ Binary conversion complete\n- Gene lists: {out_path}\n- Gene lists (essentials filled): {filled}")
    return True


def run_genome_minimizer(args):
    """main.py:528-614 (same checks, messages and output layout)."""
    from gm2.minimizer import process_multiple_genomes_multiple_files, process_multiple_genomes_single_file
    print("\n" + "=" * 80 + "\nGENOME MINIMIZER RUN\n" + "=" * 80)
    genome_path = args.genome_path or os.path.join(args.project_root, "data", "wild_type_sequence.gb")
    if not os.path.exists(genome_path):
        print(f"✗ Genome file not found: {genome_path}")
        return None
    if not args.genes_path:
        print("✗ Genes path required for genome minimizer")
        return None
    if not os.path.exists(args.genes_path):
        print(f"✗ Genes file not found: {args.genes_path}")
        return None
    print(f"\n{'=' * 80}\nProcessing genome: {Path(genome_path).name}\nUsing genes from: {Path(args.genes_path).name}"
          f"\nModel name: {args.model_name}\n{'=' * 80}")
    try:
        if args.output_file:
            output_dir, output_filename = Path(args.output_file).parent, Path(args.output_file).name
        elif args.single_file:
            output_dir, output_filename = Path(args.output_dir), f"minimized_genomes_{args.model_name}.fasta"
        else:
            output_dir, output_filename = Path(args.output_dir), None
        output_dir.mkdir(parents=True, exist_ok=True)
        print(f"✓ Created output directory: {output_dir}")
        if args.single_file or args.output_file:
            output_file = output_dir / output_filename
            print(f"Generating single FASTA file: {output_file}")
            result = process_multiple_genomes_single_file(genome_path=genome_path, genes_path=args.genes_path,
                                                          model_name=args.model_name, output_file=str(output_file))
            print("\n✓ GENOME MINIMIZATION COMPLETED!")
            print(f"- Single file generated: {output_file}")
        else:
            print(f"Generating multiple files in: {output_dir}")
            result = process_multiple_genomes_multiple_files(genome_path=genome_path, genes_path=args.genes_path,
                                                             model_name=args.model_name, output_dir=str(output_dir))
            print("\n✓ GENOME MINIMIZATION COMPLETED!")
        print(f"- Processed: {result['genome_count']} genomes")
        print(f"- Average percentage reduction: {result['average_reduction_pct']:.1f}%")
        print(f"- Average genome length: {result['average_length_bp']:,.1f} bp")
        return result
    except Exception as e:
        print(f"✗ Error during genome minimization: {e}")
        traceback.print_exc()
        return None


def main(argv=None):
    args = parse_arguments(argv)
    if args.grad_exchange:
        os.environ["GM2_GRAD_EXCHANGE"] = args.grad_exchange  # read by the trainer's gradient exchange
    if args.sync_bn:
        os.environ["GM2_SYNC_BN"] = "1"  # read by VAETrainer
    dist = None
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        # torchrun: one process per GPU; bind the device and join the process group before any
        # other GPU work (strain-row data parallelism)
        if args.mode not in ("training", "sample"):
            if int(os.environ.get("RANK", "0")) != 0:
                return 0
            print(f"--mode {args.mode} does not shard; running it on rank 0 only")
        else:
            from gm2.ddp import init_from_env
            dist = init_from_env()
    try:
        return _main(args)
    finally:
        if dist is not None:
            dist.destroy_process_group()


def _main(args):
    print(f"\nRunning in {args.mode} mode (MI355X / gfx950 build)")
    if args.mode not in IMPLEMENTED:
        print(f"✗ --mode {args.mode} is outside the MI355X hot path of this build (SURVEY.md §2); "
              "use the reference for it")
        return 2
    if args.mode not in ("convert-samples", "minimizer") and not check_data_availability(args.project_root):
        print("\n✗ Cannot proceed without required data files")
        return 1
    try:
        if args.mode == "sample":
            return 0 if run_sampling(args) else 1
        if args.mode == "convert-samples":
            return 0 if run_binary_converter(args) else 1
        if args.mode == "minimizer":
            if run_genome_minimizer(args) is None:
                return 1
            print("\n" + "=" * 80 + "\nPROCESS COMPLETED!\n" + "=" * 80)
            if args.single_file or args.output_file:
                print("- Check for the generated FASTA file\n")
            else:
                print(f"- Check the {args.output_dir}/ directory for minimized genomes\n")
            return 0
        results = run_single_experiment(args)
        if results is None:
            return 1
    except KeyboardInterrupt:
        print("\n\n✗ Process interrupted by user")
        return 1
    except Exception as e:  # main.py:686-692
        print(f"\n✗ Unexpected error: {e}")
        traceback.print_exc()
        return 1
    print("\n" + "=" * 80 + "\nPROCESS COMPLETED!\n" + "=" * 80)
    return 0


if __name__ == "__main__":
    sys.exit(main())
