#!/usr/bin/env python3
"""Times the streaming smallest-genome search on the GPU (no pass / fail: a record).

A v1-shaped checkpoint with fresh weights at G = 55,039 genes, 300 essential groups on random columns
(one in ten with two positions), the viability bound at the median essential count of a probe chunk.
Three legs, each warmed on every shape it times, timed with device events:
  * stream   gm2.search.search_smallest over --samples genomes in chunks of --chunk, keeping --keep: one
             event pair around each whole search, --reps searches, the median
  * stages   per full chunk: the chunk's decode_bits (an event pair around the call) beside the four stages
             of its push, each launch group between its own event pair inside the library
             (gm2_timing_begin, GM2_KC_SEARCH_*): score (the pass over the row bytes), dedupe (table clear,
             insert, mark), select, gather; medians over the timed chunks
  * parent   the route without the search at the same N: decode_bits of all N genomes, row_sizes,
             count_groups, to_host (the masks cross PCIe), --reps times, the median
Prints one JSON line and writes a readable record to profiles/search_stream.txt.

  python tools/search_bench.py [--samples 1000000 --chunk 65536 --keep 1024 --genes 55039 --reps 3]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome-minimizer-2_amd"))


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def timed(fn, reps, torch):
    """Milliseconds of each of `reps` calls of fn, each between its own pair of device events."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--keep", type=int, default=1024)
    ap.add_argument("--genes", type=int, default=55039)
    ap.add_argument("--groups", type=int, default=300)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--stage-chunks", type=int, default=8)
    ap.add_argument("--skip-parent", action="store_true", help="leave out the all-at-once route (it holds N masks)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_stream.txt"))
    a = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("search_bench: needs the GPU (a host run measures nothing)")
    from gm2 import native
    from gm2.experiments import PRESETS
    from gm2.masks import PackedMasks
    from gm2.model import VAE
    from gm2.search import SmallestSearch, search_smallest

    cfg = PRESETS["v1"]()
    G, L, N, C, K = a.genes, cfg.latent_dim, a.samples, a.chunk, a.keep
    torch.manual_seed(0)
    model = VAE(G, cfg.hidden_dim, L)
    model.eval()
    rng = np.random.Generator(np.random.PCG64(1))
    cols = rng.choice(G, size=a.groups + a.groups // 10, replace=False)
    ess = {f"g{i}": [int(cols[i])] + ([int(cols[a.groups + i // 10])] if i % 10 == 0 else []) for i in range(a.groups)}
    dev = model.device
    gen = torch.Generator(device=dev)

    # the bound: the median essential count of one probe chunk (fresh weights carry no biology)
    gen.manual_seed(7)
    probe, _ = model.decode_bits(torch.randn(min(C, N), L, device=dev, generator=gen), chunk=C)
    counts = probe.count_groups(ess)
    bound = int(np.median(counts))
    del probe
    res = {"device": torch.cuda.get_device_name(0), "genes": G, "hidden": cfg.hidden_dim, "latent": L, "samples": N,
           "chunk": C, "keep": K, "groups": a.groups, "min_essential": bound, "reps": a.reps,
           "row_bytes": native.packed_row_bytes(G)}

    # ---- stream: the whole search ----
    def stream():
        gen.manual_seed(11)
        return search_smallest(model, N, K, ess, bound, chunk=C, generator=gen, return_search=True)
    stream()
    torch.cuda.synchronize()
    t = timed(stream, a.reps, torch)
    r = stream().result()
    res["stream_ms"] = median(t)
    res["stream_ms_all"] = t
    res["stream_genomes_per_s"] = N / (median(t) * 1e-3)
    res["stream_viable"], res["stream_kept"] = r.viable, len(r.indices)
    res["stream_kept_size_range"] = [int(r.sizes.min()), int(r.sizes.max())] if len(r.indices) else None

    # ---- stages: decode of a chunk against the stages of its push ----
    n_c = min(C, N)
    search = SmallestSearch(G, K, ess, bound, latent_dim=L, device=dev, chunk_max=n_c)
    buf = PackedMasks.empty(n_c, G, dev)
    classes = {"score": native.KC_SEARCH_SCORE, "dedupe": native.KC_SEARCH_DEDUPE, "select": native.KC_SEARCH_SELECT,
               "gather": native.KC_SEARCH_GATHER}
    stage = {k: [] for k in classes}
    decode_ms, push_ms = [], []
    gen.manual_seed(13)
    for it in range(2 + a.stage_chunks):       # (two warm-up chunks: the first fills the state)
        z = torch.randn(n_c, L, device=dev, generator=gen)
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        masks, _ = model.decode_bits(z, chunk=C, out=buf)
        e[1].record()
        native.timing_begin(sum(classes.values()))
        search.push(masks, z)
        e[2].record()
        native.timing_end()
        torch.cuda.synchronize()
        if it >= 2:
            decode_ms.append(e[0].elapsed_time(e[1]))
            push_ms.append(e[1].elapsed_time(e[2]))
            for k, c in classes.items():
                stage[k].append(native.timing_class(c)[0])
    res["chunk_rows"] = n_c
    res["chunk_decode_ms"] = median(decode_ms)
    res["chunk_push_ms"] = median(push_ms)
    res["chunk_stage_ms"] = {k: median(v) for k, v in stage.items()}
    res["chunk_stages_over_decode"] = sum(res["chunk_stage_ms"].values()) / res["chunk_decode_ms"]
    res["chunk_score_tb_per_s"] = n_c * res["row_bytes"] / (res["chunk_stage_ms"]["score"] * 1e-3) / 1e12

    # ---- parent: everything at once, masks to the host ----
    if not a.skip_parent:
        def parent():
            gen.manual_seed(11)
            z = torch.randn(N, L, device=dev, generator=gen)
            p, _ = model.decode_bits(z, chunk=C)
            sizes = p.row_sizes()
            ce = p.count_groups(ess)
            host = p.to_host()
            return sizes, ce, host
        parent()
        torch.cuda.synchronize()
        t = timed(parent, a.reps, torch)
        res["parent_ms"] = median(t)
        res["parent_ms_all"] = t
        res["parent_genomes_per_s"] = N / (median(t) * 1e-3)
        res["parent_over_stream"] = res["parent_ms"] / res["stream_ms"]
        res["parent_device_mask_bytes"] = N * res["row_bytes"]

    lines = [f"streaming smallest-genome search, {res['device']}",
             f"v1-shaped fresh model {G} -> {cfg.hidden_dim} -> {L}; N = {N}, chunk = {C}, keep = {K}, "
             f"{a.groups} essential groups, bound {bound}; medians of {a.reps} runs, device events",
             f"stream   {res['stream_ms']:.1f} ms  ({res['stream_genomes_per_s'] / 1e6:.2f} M genomes/s; "
             f"{res['stream_viable']} viable, kept {res['stream_kept']}, sizes {res['stream_kept_size_range']})",
             f"chunk of {n_c}: decode_bits {res['chunk_decode_ms']:.3f} ms, push {res['chunk_push_ms']:.3f} ms"]
    lines += [f"  {k:<7}{v:.3f} ms" for k, v in res["chunk_stage_ms"].items()]
    lines += [f"  stages / decode = {res['chunk_stages_over_decode']:.4f}; score reads "
              f"{res['chunk_score_tb_per_s']:.2f} TB/s of row bytes"]
    if not a.skip_parent:
        lines += [f"parent   {res['parent_ms']:.1f} ms  ({res['parent_genomes_per_s'] / 1e6:.2f} M genomes/s; decode all + row_sizes + "
                  f"count_groups + to_host; {res['parent_device_mask_bytes'] / 1e9:.2f} GB of masks on the device and over "
                  f"PCIe); parent / stream = {res['parent_over_stream']:.2f}"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n" + json.dumps(res) + "\n")
    print("\n".join(lines))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
