#!/usr/bin/env python3
"""Record the eval render loop's schedule -> tests/golden/render_loop_schedule.json: what the host chose at every
read-back (`_loop_debug`) with the native pair call, and what every iteration of the per-stage loop was issued with (`_loop_probe`: lanes,
rows, n_total and the alive count of the iteration's state snapshot).  Scene of tests/test_gpu_pipeline.py::_setup(emb_scale=0.5); frames of
20000 rays (seed 3) and 4096 rays (seed 4) at density_scale 1, 40 and 300 (the last with perturb).  The golden was recorded on the commit
named in its 'parent' field, before nerf/render_loop.py existed: tests/test_render_loop_schedule.py replays its read-backs through
render_loop.Schedule, tests/test_gpu_pipeline.py compares a live frame's stages with it.

    python tools/render_loop_schedule_dump.py --parent <commit> [--out tests/golden/render_loop_schedule.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'torch-ngp_amd'))
sys.path.insert(0, ROOT)

FRAMES = ((20000, 3), (4096, 4))                       # (rays, seed)
CASES = ((1.0, False), (40.0, False), (300.0, True))   # (density_scale, perturb)
RENDER = dict(staged=True, bg_color=1, dt_gamma=0, max_steps=1024, T_thresh=1e-4)


def frame_rays(n_rays, seed, dev):
    import numpy as np
    import torch
    import synthetic_scene as sc
    rng = np.random.default_rng(seed)
    pose = sc.camera_pose(rng)
    o, d = sc.rays_for_pixels(pose, rng.integers(0, sc.RES * sc.RES, n_rays))
    return torch.from_numpy(o)[None].to(dev), torch.from_numpy(d)[None].to(dev)


def record(model, rays, density_scale, perturb, native):
    """one frame -> {'debug': the _loop_debug tuples, 'final_alive', 'device_rows'} and, for the per-stage loop (native = False),
    'iterations': [lanes, rows, n_total, alive] per iteration and 'stages': the stage names of an iteration (the same in every one)"""
    import torch
    model.eval()
    model.density_scale = density_scale
    model.device_loop, model.graph_loop, model.native_loop = True, False, native
    model._loop_cache, model._loop_debug, model._loop_probe = None, [], None if native else []
    torch.manual_seed(5)
    with torch.no_grad(), torch.autocast('cuda', dtype=torch.float16):
        model.render(*rays, perturb=perturb, **RENDER)
    torch.cuda.synchronize()
    out = {'debug': [list(t) for t in model._loop_debug], 'final_alive': int(model._loop_cache['state'][0, 0].item()),
           'device_rows': 'rows_used' in model._loop_cache}
    if not native:
        out['iterations'], names = [], []
        for name, _, _, lanes, rows, n_total, snap in model._loop_probe:
            entry = [lanes, rows, n_total, int(snap[0].item())]
            if not out['iterations'] or snap is not last:
                out['iterations'].append(entry)
                names.append([])
            last = snap
            names[-1].append(name)
        assert all(n == names[0] for n in names), names
        out['stages'] = names[0]
    model._loop_debug = model._loop_probe = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', required=True, help='the commit this is recorded on')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'render_loop_schedule.json'))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import torch
    from test_gpu_pipeline import _setup
    model, _, _, dev = _setup(emb_scale=0.5)
    frames = []
    for n_rays, seed in FRAMES:
        rays = frame_rays(n_rays, seed, dev)
        for density_scale, perturb in CASES:
            frames.append({'n_rays': n_rays, 'seed': seed, 'density_scale': density_scale, 'perturb': perturb,
                           'native': record(model, rays, density_scale, perturb, True),
                           'stages': record(model, rays, density_scale, perturb, False)})
    doc = {'parent': args.parent, 'device': torch.cuda.get_device_name(0), 'render': RENDER, 'frames': frames}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(json.dumps(doc, separators=(',', ':')).replace('{"n_rays"', '\n{"n_rays"') + '\n')
    print('wrote', args.out, len(frames), 'frames')


if __name__ == '__main__':
    main()
