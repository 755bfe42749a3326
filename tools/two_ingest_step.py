"""What a pipeline that ingests AGAIN pays for planes its first scatter left in the bands.
One step = a fresh pipeline, INGESTS ingests of the workload's cloud into it, finalize; prints one JSON line with the
median / min / max step time over STEPS steps (pipelines are created ahead of the clock, as bench.py does).
Run on the GPU box: python tools/two_ingest_step.py [workload=C2] [ingests=2] [steps=16] [warmup=4]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401
import bench
bench._imports()                                   # bench imports torch / pcr lazily (its launcher branch must not)
from bench import pcr, ShardedPipeline, make_points, make_cloud, make_specs

wl = sys.argv[1] if len(sys.argv) > 1 else "C2"
ingests, steps, warmup = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 2), (3, 16), (4, 4)))
G, n = 4096, 50_000_000
cfg = pcr.PipelineConfig()
cfg.grid.bounds = pcr.BBox(0.0, 0.0, float(G), float(G))
cfg.grid.cell_size_x, cfg.grid.cell_size_y = 1.0, -1.0
cfg.grid.compute_dimensions()
cfg.exec_mode = pcr.ExecutionMode.GPU
cfg.reductions = make_specs(wl)
cfg.result_location = pcr.MemoryLocation.Device
cfg.gpu_pool_size_bytes = 16 * n + (64 << 20)
x, y, v, ch = make_points(wl, n, G, 0.0, float(G), seed=42)
cloud = make_cloud(x, y, v, ch).to_device()
times = []
for chunk in (warmup, steps):
    pipes = [ShardedPipeline(cfg, 0, 1, device_id=0) for _ in range(chunk)]
    for sp in pipes:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(ingests):
            sp.pipe.ingest(cloud)
        sp.finalize()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    info = pipes[-1].pipe.last_scatter()
    pipes = None
ms = sorted(1e3 * t for t in times[warmup:])
print(json.dumps({"workload": wl, "ingests": ingests, "steps": steps, "ms_per_step_median": round(ms[len(ms) // 2], 4),
                  "ms_per_step_min": round(ms[0], 4), "ms_per_step_max": round(ms[-1], 4), "last_scatter": info}))
