"""Cost of mesh extraction (csrc/surface_nets.hip, NeRFRenderer.extract_mesh) per lattice resolution, for a density model
(nerf/network_ff.py, random table, the synthetic scene's occupancy grid) and a NeuSNetwork at initialisation (occupancy refreshed from its own
density):
  kept            the fraction of lattice points raymarching.lattice_points keeps (one occupancy cell of dilation)
  fill            NeRFRenderer.mesh_volume dense against culled -- the same process, alternating inside every repetition, host clock around
                  work that ends in a device synchronisation (the fill reads one count back per slab anyway)
  count / emit    device time (HIP events) of ngp_surface_nets_count (two launches) and ngp_surface_nets_emit (two launches and the
                  read-back of the counts) on the culled volume, and the bytes of ONE volume read (4 B per lattice point) over each time --
                  next to the 6.3 TB/s copy ceiling DESIGN.md section 9 quotes for k_adam.  count reads the volume once through L1 / L2 (every
                  point is a corner of eight cells); emit reads it twice (vertices: eight corners, faces: four) and writes the mesh.
One JSON line per (model, resolution).

    python tools/bench_extract_mesh.py [--resolution 256 512] [--iters 5] [--warmup 1]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'torch-ngp_amd'), ROOT]

import torch  # noqa: E402

COPY_CEILING_TB_S = 6.3


def density_model(dev):
    import raymarching
    import synthetic_scene as sc
    from nerf.network_ff import NeRFNetwork
    torch.manual_seed(0)
    model = NeRFNetwork(bound=1, cuda_ray=True, density_scale=1).to(dev)
    with torch.no_grad():
        model.encoder.embeddings.uniform_(-0.5, 0.5)
        model.density_grid.copy_(torch.from_numpy(sc.occupancy_density()))
    model.density_bitfield = raymarching.packbits(model.density_grid, 10.0, model.density_bitfield)
    return model


def sdf_model(dev):
    from nerf.network_sdf import NeuSNetwork
    torch.manual_seed(0)
    model = NeuSNetwork(bound=1, cuda_ray=True, prior_radius=0.5).to(dev)
    with torch.autocast('cuda', dtype=torch.float16):
        model.update_extra_state()
    return model


def _host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def _device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def measure(name, model, res, iters, warmup):
    import raymarching
    from raymarching import backend as be
    dims = (res, res, res)
    lo, hi = -model.bound, model.bound
    fills = {'dense': [], 'culled': []}
    evaluated = {}
    for it in range(warmup + iters):
        for kind in fills:                      # alternate the candidates inside every repetition
            ms, (volume, n) = _host_ms(lambda: model.mesh_volume(dims, lo, hi, cull=kind == 'culled'))
            evaluated[kind] = n
            if it >= warmup:
                fills[kind].append(ms)
            if kind == 'dense':
                del volume                      # (two 512^3 volumes and their slabs need not coexist)
    level, below = model.mesh_level, model.mesh_inside_below
    origin, spacing = raymarching.lattice_frame(lo, hi, dims)
    ws = be.surface_nets_workspace(volume)
    counts = torch.empty(2, dtype=torch.int32, device=volume.device)
    be.surface_nets_count(volume, level, below, ws, counts)
    n_v, n_f = counts.tolist()
    vertices = torch.empty(max(n_v, 1), 3, device=volume.device)
    faces = torch.empty(max(n_f, 1), 3, dtype=torch.int32, device=volume.device)
    count_ms, emit_ms = [], []
    for it in range(warmup + iters):
        c = _device_ms(lambda: be.surface_nets_count(volume, level, below, ws, counts))
        e = _device_ms(lambda: be.surface_nets_emit(volume, level, below, origin, spacing, ws, vertices, faces))
        if it >= warmup:
            count_ms.append(c)
            emit_ms.append(e)
    med = lambda v: statistics.median(v)
    volume_bytes = 4 * res ** 3
    out = {'model': name, 'resolution': res, 'lattice_points': res ** 3, 'kept_fraction': round(evaluated['culled'] / res ** 3, 4),
           'fill_dense_ms': round(med(fills['dense']), 2), 'fill_culled_ms': round(med(fills['culled']), 2),
           'fill_dense_over_culled': round(med(fills['dense']) / med(fills['culled']), 2),
           'vertices': n_v, 'triangles': n_f, 'count_ms': round(med(count_ms), 3), 'emit_ms': round(med(emit_ms), 3),
           'volume_bytes': volume_bytes,
           'count_volume_tb_per_s': round(volume_bytes / (med(count_ms) * 1e-3) / 1e12, 3),
           'emit_volume_tb_per_s': round(volume_bytes / (med(emit_ms) * 1e-3) / 1e12, 3),
           'copy_ceiling_tb_per_s': COPY_CEILING_TB_S, 'iters': iters}
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_extract_mesh needs a GPU: a CPU run gives no time')
    dev = torch.device('cuda')
    for name, build in (('density', density_model), ('sdf', sdf_model)):
        model = build(dev)
        for res in args.resolution:
            measure(name, model, res, args.iters, args.warmup)
        del model
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
