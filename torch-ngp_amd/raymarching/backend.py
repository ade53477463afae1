"""`_backend` of the ray marcher: the ten callables of raymarching/src/bindings.cpp:5-19 over
libngp_hip.so, plus `compact_rays` (device-side stream compaction, an extension declared in
include/ngp_hip.h).  Argument order is the reference's (raymarching/src/raymarching.h:7-18)."""
import types

import torch

import _ngp_capi as capi


def _f32(t, name):
    capi.dense(t, name)
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be a float32 tensor (the reference wrappers cast with custom_fwd(cast_inputs=float32))")
    return t


def _f64(pairs):
    """float64 call of an entry with an fp64 twin (include/ngp_hip.h, *_f64): True when one floating tensor is float64 -- then all must be,
    contiguous and on the device"""
    if not capi.float64_call(*pairs):
        return False
    for t, n in pairs:
        capi.dense(t, n)
    return True


def _f32_call(pairs, fn):
    for t, n in pairs:
        _f32(t, n)
    return fn


def _i32(t, name):
    capi.dense(t, name)
    capi.require_int32(t, name)
    return t


def near_far_from_aabb(rays_o, rays_d, aabb, N, min_near, nears, fars):
    floats = ((rays_o, 'rays_o'), (rays_d, 'rays_d'), (aabb, 'aabb'), (nears, 'nears'), (fars, 'fars'))
    fn = capi.lib.ngp_near_far_from_aabb_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_near_far_from_aabb)
    capi.check(fn(capi.ptr(rays_o), capi.ptr(rays_d), capi.ptr(aabb), N, float(min_near), capi.ptr(nears), capi.ptr(fars), capi.stream()))


def sph_from_ray(rays_o, rays_d, radius, N, coords):
    floats = ((rays_o, 'rays_o'), (rays_d, 'rays_d'), (coords, 'coords'))
    fn = capi.lib.ngp_sph_from_ray_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_sph_from_ray)
    capi.check(fn(capi.ptr(rays_o), capi.ptr(rays_d), float(radius), N, capi.ptr(coords), capi.stream()))


def morton3D(coords, N, indices):
    _i32(coords, 'coords'); _i32(indices, 'indices')
    capi.check(capi.lib.ngp_morton3D(capi.ptr(coords), N, capi.ptr(indices), capi.stream()))


def morton3D_invert(indices, N, coords):
    _i32(coords, 'coords'); _i32(indices, 'indices')
    capi.check(capi.lib.ngp_morton3D_invert(capi.ptr(indices), N, capi.ptr(coords), capi.stream()))


def packbits(grid, N, density_thresh, bitfield):
    floats = ((grid, 'grid'),)
    fn = capi.lib.ngp_packbits_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_packbits)
    capi.dense(bitfield, 'bitfield')
    if bitfield.dtype != torch.uint8:
        raise RuntimeError("bitfield must be a uint8 tensor")
    capi.check(fn(capi.ptr(grid), N, float(density_thresh), capi.ptr(bitfield), capi.stream()))


def packbits_capped(grid, N, density_thresh, thresh_cap, bitfield):
    """extension: threshold = min(density_thresh, thresh_cap[0]) with thresh_cap a device scalar (include/ngp_hip.h, ngp_packbits_ex)"""
    capi.check(capi.lib.ngp_packbits_ex(capi.ptr(grid), N, float(density_thresh), capi.ptr(thresh_cap), capi.ptr(bitfield), capi.stream()))


def density_grid_update(sigmas, cells, n, density_scale, decay, density_grid, n_cells, scratch, density_thresh, mean_out, bitfield, workspace):
    """extension: the apply half of the occupancy refresh in three launches (include/ngp_hip.h, ngp_density_grid_update)"""
    _f32(sigmas, 'sigmas'); _f32(density_grid, 'density_grid'); _f32(scratch, 'scratch'); _f32(mean_out, 'mean_out')
    capi.dense(cells, 'cells')
    if cells.dtype != torch.int64:
        raise RuntimeError("cells must be an int64 tensor")
    capi.check(capi.lib.ngp_density_grid_update(capi.ptr(sigmas), capi.ptr(cells), n, float(density_scale), float(decay), capi.ptr(density_grid),
                                                n_cells, capi.ptr(scratch), float(density_thresh), capi.ptr(mean_out), capi.ptr(bitfield),
                                                capi.ptr(workspace), capi.stream()))


def density_grid_update_workspace_bytes(n_cells):
    return int(capi.lib.ngp_density_grid_update_workspace_bytes(n_cells))


def march_rays_train(rays_o, rays_d, grid, bound, dt_gamma, max_steps, N, C, H, M, nears, fars, xyzs, dirs, deltas, rays,
                     counter, noises):
    for t, n in ((rays_o, 'rays_o'), (rays_d, 'rays_d'), (nears, 'nears'), (fars, 'fars'), (xyzs, 'xyzs'), (dirs, 'dirs'),
                 (deltas, 'deltas'), (noises, 'noises')):
        _f32(t, n)
    _i32(rays, 'rays'); _i32(counter, 'counter')
    capi.dense(grid, 'grid')
    ws = torch.empty(capi.lib.ngp_march_rays_train_workspace_bytes(N), dtype=torch.uint8, device=rays_o.device)
    capi.check(capi.lib.ngp_march_rays_train(
        capi.ptr(rays_o), capi.ptr(rays_d), capi.ptr(grid), float(bound), float(dt_gamma), max_steps, N, C, H, M,
        capi.ptr(nears), capi.ptr(fars), capi.ptr(xyzs), capi.ptr(dirs), capi.ptr(deltas), capi.ptr(rays), capi.ptr(counter),
        capi.ptr(noises), capi.ptr(ws), capi.stream()))


def composite_rays_train_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image):
    floats = ((sigmas, 'sigmas'), (rgbs, 'rgbs'), (deltas, 'deltas'), (weights_sum, 'weights_sum'), (depth, 'depth'), (image, 'image'))
    fn = capi.lib.ngp_composite_rays_train_forward_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_composite_rays_train_forward)
    _i32(rays, 'rays')
    capi.check(fn(capi.ptr(sigmas), capi.ptr(rgbs), capi.ptr(deltas), capi.ptr(rays), M, N, float(T_thresh), capi.ptr(weights_sum), capi.ptr(depth),
                  capi.ptr(image), capi.stream()))


def composite_rays_train_backward(grad_weights_sum, grad_image, sigmas, rgbs, deltas, rays, weights_sum, image, M, N, T_thresh,
                                  grad_sigmas, grad_rgbs):
    floats = ((grad_weights_sum, 'grad_weights_sum'), (grad_image, 'grad_image'), (sigmas, 'sigmas'), (rgbs, 'rgbs'), (deltas, 'deltas'),
              (weights_sum, 'weights_sum'), (image, 'image'), (grad_sigmas, 'grad_sigmas'), (grad_rgbs, 'grad_rgbs'))
    fn = capi.lib.ngp_composite_rays_train_backward_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_composite_rays_train_backward)
    _i32(rays, 'rays')
    capi.check(fn(
        capi.ptr(grad_weights_sum), capi.ptr(grad_image), capi.ptr(sigmas), capi.ptr(rgbs), capi.ptr(deltas), capi.ptr(rays),
        capi.ptr(weights_sum), capi.ptr(image), M, N, float(T_thresh), capi.ptr(grad_sigmas), capi.ptr(grad_rgbs), capi.stream()))


def composite_rays_train_geo_forward(sigmas, rgbs, deltas, rays, M, N, T_thresh, weights_sum, depth, image, distortion):
    """extension (include/ngp_hip.h, ngp_composite_rays_train_geo_forward): composite_rays_train_forward + the per-ray distortion.  Not in
    the compiled `_raymarching` module (its table is the reference's): raymarching.py calls this helper whichever backend it imported."""
    floats = ((sigmas, 'sigmas'), (rgbs, 'rgbs'), (deltas, 'deltas'), (weights_sum, 'weights_sum'), (depth, 'depth'), (image, 'image'),
              (distortion, 'distortion'))
    fn = capi.lib.ngp_composite_rays_train_geo_forward_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_composite_rays_train_geo_forward)
    _i32(rays, 'rays')
    capi.check(fn(capi.ptr(sigmas), capi.ptr(rgbs), capi.ptr(deltas), capi.ptr(rays), M, N, float(T_thresh), capi.ptr(weights_sum), capi.ptr(depth),
                  capi.ptr(image), capi.ptr(distortion), capi.stream()))


def composite_rays_train_geo_backward(grad_weights_sum, grad_depth, grad_image, grad_distortion, sigmas, rgbs, deltas, rays, weights_sum, depth,
                                      image, distortion, M, N, T_thresh, grad_sigmas, grad_rgbs):
    """extension (ngp_composite_rays_train_geo_backward): the gradients of all four outputs in one sweep; a None gradient is a zero one"""
    floats = tuple((t, n) for t, n in (
        (grad_weights_sum, 'grad_weights_sum'), (grad_depth, 'grad_depth'), (grad_image, 'grad_image'), (grad_distortion, 'grad_distortion'),
        (sigmas, 'sigmas'), (rgbs, 'rgbs'), (deltas, 'deltas'), (weights_sum, 'weights_sum'), (depth, 'depth'), (image, 'image'),
        (distortion, 'distortion'), (grad_sigmas, 'grad_sigmas'), (grad_rgbs, 'grad_rgbs')) if t is not None)
    fn = capi.lib.ngp_composite_rays_train_geo_backward_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_composite_rays_train_geo_backward)
    _i32(rays, 'rays')
    capi.check(fn(
        capi.ptr(grad_weights_sum), capi.ptr(grad_depth), capi.ptr(grad_image), capi.ptr(grad_distortion), capi.ptr(sigmas), capi.ptr(rgbs),
        capi.ptr(deltas), capi.ptr(rays), capi.ptr(weights_sum), capi.ptr(depth), capi.ptr(image), capi.ptr(distortion), M, N, float(T_thresh),
        capi.ptr(grad_sigmas), capi.ptr(grad_rgbs), capi.stream()))


def composite_rays_train_features_forward(sigmas, feats, deltas, rays, M, N, C, T_thresh, out):
    """extension (include/ngp_hip.h, ngp_composite_rays_train_features_forward): out [N,C] = the composite of the per-sample channels feats
    [M,C].  float64 everywhere, or sigmas / deltas / out float32 with feats float32 or float16 (converted at the load).  ctypes-only, like the
    geometry compositor's entries."""
    _i32(rays, 'rays')
    if _f64(((sigmas, 'sigmas'), (feats, 'feats'), (deltas, 'deltas'), (out, 'out'))):
        capi.check(capi.lib.ngp_composite_rays_train_features_forward_f64(capi.ptr(sigmas), capi.ptr(feats), capi.ptr(deltas), capi.ptr(rays), M, N, C,
                                                                          float(T_thresh), capi.ptr(out), capi.stream()))
        return
    for t, n in ((sigmas, 'sigmas'), (deltas, 'deltas'), (out, 'out')):
        _f32(t, n)
    capi.check(capi.lib.ngp_composite_rays_train_features_forward(capi.ptr(sigmas), capi.ptr(capi.dense(feats, 'feats')), capi.ptr(deltas),
                                                                  capi.ptr(rays), M, N, C, float(T_thresh), _feat_code(feats, 'feats'), capi.ptr(out),
                                                                  capi.stream()))


def composite_rays_train_features_backward(grad_out, sigmas, feats, deltas, rays, out, M, N, C, T_thresh, grad_sigmas, grad_feats):
    """extension (ngp_composite_rays_train_features_backward): grad_sigmas [M] and grad_feats [M,C] (the dtype of feats), pre-zeroed by the
    caller -- rows no ray composites are not written"""
    _i32(rays, 'rays')
    if _f64(((grad_out, 'grad_out'), (sigmas, 'sigmas'), (feats, 'feats'), (deltas, 'deltas'), (out, 'out'), (grad_sigmas, 'grad_sigmas'),
             (grad_feats, 'grad_feats'))):
        capi.check(capi.lib.ngp_composite_rays_train_features_backward_f64(
            capi.ptr(grad_out), capi.ptr(sigmas), capi.ptr(feats), capi.ptr(deltas), capi.ptr(rays), capi.ptr(out), M, N, C, float(T_thresh),
            capi.ptr(grad_sigmas), capi.ptr(grad_feats), capi.stream()))
        return
    for t, n in ((grad_out, 'grad_out'), (sigmas, 'sigmas'), (deltas, 'deltas'), (out, 'out'), (grad_sigmas, 'grad_sigmas')):
        _f32(t, n)
    capi.dense(feats, 'feats'); capi.dense(grad_feats, 'grad_feats')
    if grad_feats.dtype != feats.dtype:
        raise RuntimeError(f"grad_feats must have the dtype of feats ({feats.dtype}, got {grad_feats.dtype})")
    capi.check(capi.lib.ngp_composite_rays_train_features_backward(
        capi.ptr(grad_out), capi.ptr(sigmas), capi.ptr(feats), capi.ptr(deltas), capi.ptr(rays), capi.ptr(out), M, N, C, float(T_thresh),
        _feat_code(feats, 'feats'), capi.ptr(grad_sigmas), capi.ptr(grad_feats), capi.stream()))


def _feat_code(t, name):
    if t.dtype not in (torch.float32, torch.float16):
        raise RuntimeError(f"{name} must be a float32 or float16 tensor (got {t.dtype})")
    return capi.float_code(t, name)


def march_rays(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, nears, fars, xyzs, dirs,
               deltas, noises):
    for t, n in ((rays_t, 'rays_t'), (rays_o, 'rays_o'), (rays_d, 'rays_d'), (nears, 'nears'), (fars, 'fars'), (xyzs, 'xyzs'),
                 (dirs, 'dirs'), (deltas, 'deltas'), (noises, 'noises')):
        _f32(t, n)
    _i32(rays_alive, 'rays_alive')
    capi.dense(grid, 'grid')
    capi.check(capi.lib.ngp_march_rays(n_alive, n_step, capi.ptr(rays_alive), capi.ptr(rays_t), capi.ptr(rays_o), capi.ptr(rays_d),
                                       float(bound), float(dt_gamma), max_steps, C, H, capi.ptr(grid), capi.ptr(nears), capi.ptr(fars),
                                       capi.ptr(xyzs), capi.ptr(dirs), capi.ptr(deltas), capi.ptr(noises), capi.stream()))


def march_rays_ex(n_alive, n_step, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, nears, fars, xyzs, dirs,
                  deltas, noises, zero_rows):
    """extension: as march_rays, but the kernel zeroes the slots it does not fill (buffers may be torch.empty) and noises may be None"""
    for t, n in ((rays_t, 'rays_t'), (rays_o, 'rays_o'), (rays_d, 'rays_d'), (nears, 'nears'), (fars, 'fars'), (xyzs, 'xyzs'),
                 (dirs, 'dirs'), (deltas, 'deltas')):
        _f32(t, n)
    if noises is not None:
        _f32(noises, 'noises')
    _i32(rays_alive, 'rays_alive')
    capi.dense(grid, 'grid')
    capi.check(capi.lib.ngp_march_rays_ex(n_alive, n_step, capi.ptr(rays_alive), capi.ptr(rays_t), capi.ptr(rays_o), capi.ptr(rays_d),
                                          float(bound), float(dt_gamma), max_steps, C, H, capi.ptr(grid), capi.ptr(nears), capi.ptr(fars),
                                          capi.ptr(xyzs), capi.ptr(dirs), capi.ptr(deltas), capi.ptr(noises), zero_rows, capi.stream()))


def composite_rays(n_alive, n_step, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image):
    floats = ((rays_t, 'rays_t'), (sigmas, 'sigmas'), (rgbs, 'rgbs'), (deltas, 'deltas'), (weights_sum, 'weights_sum'), (depth, 'depth'),
              (image, 'image'))
    fn = capi.lib.ngp_composite_rays_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_composite_rays)
    _i32(rays_alive, 'rays_alive')
    capi.check(fn(n_alive, n_step, float(T_thresh), capi.ptr(rays_alive), capi.ptr(rays_t), capi.ptr(sigmas), capi.ptr(rgbs), capi.ptr(deltas),
                  capi.ptr(weights_sum), capi.ptr(depth), capi.ptr(image), capi.stream()))


def compact_rays(rays_alive, n_alive, out_alive, out_count):
    _i32(rays_alive, 'rays_alive'); _i32(out_alive, 'out_alive'); _i32(out_count, 'out_count')
    ws = torch.empty(capi.lib.ngp_compact_rays_workspace_bytes(n_alive), dtype=torch.uint8, device=rays_alive.device)
    capi.check(capi.lib.ngp_compact_rays(capi.ptr(rays_alive), n_alive, capi.ptr(out_alive), capi.ptr(out_count), capi.ptr(ws),
                                         capi.stream()))


def coarse_occupancy(grid, C, H, coarse):
    """extension (include/ngp_hip.h): dilated (H/4)^3 occupancy per cascade, for cull_rays"""
    capi.dense(grid, 'grid'); capi.dense(coarse, 'coarse')
    if coarse.numel() * coarse.element_size() < capi.lib.ngp_coarse_occupancy_bytes(C, H):
        raise RuntimeError('coarse_occupancy: `coarse` is too small')
    capi.check(capi.lib.ngp_coarse_occupancy(capi.ptr(grid), C, H, capi.ptr(coarse), capi.stream()))


def cull_rays(rays_o, rays_d, nears, fars, N, bound, C, H, coarse, rays_alive):
    """extension: rays_alive[n] = n, or -1 for a ray whose [near, far] segment provably meets no occupied voxel"""
    for t, n in ((rays_o, 'rays_o'), (rays_d, 'rays_d'), (nears, 'nears'), (fars, 'fars')):
        _f32(t, n)
    _i32(rays_alive, 'rays_alive'); capi.dense(coarse, 'coarse')
    capi.check(capi.lib.ngp_cull_rays(capi.ptr(rays_o), capi.ptr(rays_d), capi.ptr(nears), capi.ptr(fars), N, float(bound), C, H, capi.ptr(coarse),
                                      capi.ptr(rays_alive), capi.stream()))


def march_rays_dev(state, alive_bound, n_total, n_step_cap, rays_alive, rays_t, rays_o, rays_d, bound, dt_gamma, max_steps, C, H, grid, nears, fars,
                   xyzs, dirs, deltas, noises, rows):
    """extension (include/ngp_hip.h, on-device inference loop): march_rays with the alive count / n_step taken from the device `state`"""
    for t, n in ((rays_t, 'rays_t'), (rays_o, 'rays_o'), (rays_d, 'rays_d'), (nears, 'nears'), (fars, 'fars'), (xyzs, 'xyzs'),
                 (dirs, 'dirs'), (deltas, 'deltas')):
        _f32(t, n)
    _i32(rays_alive, 'rays_alive'); _i32(state, 'state')
    capi.dense(grid, 'grid')
    capi.check(capi.lib.ngp_march_rays_dev(capi.ptr(state), alive_bound, n_total, n_step_cap, capi.ptr(rays_alive), capi.ptr(rays_t), capi.ptr(rays_o),
                                           capi.ptr(rays_d), float(bound), float(dt_gamma), max_steps, C, H, capi.ptr(grid), capi.ptr(nears),
                                           capi.ptr(fars), capi.ptr(xyzs), capi.ptr(dirs), capi.ptr(deltas), capi.ptr(noises), rows, capi.stream()))


def composite_rays_dev(state, alive_bound, n_total, n_step_cap, T_thresh, rays_alive, rays_t, sigmas, rgbs, deltas, weights_sum, depth, image):
    for t, n in ((rays_t, 'rays_t'), (sigmas, 'sigmas'), (rgbs, 'rgbs'), (deltas, 'deltas'), (weights_sum, 'weights_sum'),
                 (depth, 'depth'), (image, 'image')):
        _f32(t, n)
    _i32(rays_alive, 'rays_alive'); _i32(state, 'state')
    capi.check(capi.lib.ngp_composite_rays_dev(capi.ptr(state), alive_bound, n_total, n_step_cap, float(T_thresh), capi.ptr(rays_alive), capi.ptr(rays_t),
                                               capi.ptr(sigmas), capi.ptr(rgbs), capi.ptr(deltas), capi.ptr(weights_sum), capi.ptr(depth),
                                               capi.ptr(image), capi.stream()))


def composite_rays_features(n_alive, n_step, T_thresh, rays_alive, sigmas, feats, deltas, weights_sum, out):
    """extension (include/ngp_hip.h, ngp_composite_rays_features): out [N,C] += the composite of feats [>= n_alive * n_step, C] (float32 or
    float16, converted at the load) over the samples composite_rays is about to composite -- called BEFORE it on the same rows.  ctypes-only,
    like the training feature entries."""
    for t, n in ((sigmas, 'sigmas'), (deltas, 'deltas'), (weights_sum, 'weights_sum'), (out, 'out')):
        _f32(t, n)
    _i32(rays_alive, 'rays_alive')
    capi.check(capi.lib.ngp_composite_rays_features(n_alive, n_step, float(T_thresh), capi.ptr(rays_alive), capi.ptr(sigmas),
                                                    capi.ptr(capi.dense(feats, 'feats')), capi.ptr(deltas), capi.ptr(weights_sum), out.shape[-1],
                                                    _feat_code(feats, 'feats'), capi.ptr(out), capi.stream()))


def composite_rays_features_dev(state, alive_bound, n_total, n_step_cap, T_thresh, rays_alive, sigmas, feats, deltas, weights_sum, out):
    """extension (ngp_composite_rays_features_dev): composite_rays_features with the alive count / n_step taken from the device `state`"""
    for t, n in ((sigmas, 'sigmas'), (deltas, 'deltas'), (weights_sum, 'weights_sum'), (out, 'out')):
        _f32(t, n)
    _i32(rays_alive, 'rays_alive'); _i32(state, 'state')
    capi.check(capi.lib.ngp_composite_rays_features_dev(capi.ptr(state), alive_bound, n_total, n_step_cap, float(T_thresh), capi.ptr(rays_alive),
                                                        capi.ptr(sigmas), capi.ptr(capi.dense(feats, 'feats')), capi.ptr(deltas),
                                                        capi.ptr(weights_sum), out.shape[-1], _feat_code(feats, 'feats'), capi.ptr(out),
                                                        capi.stream()))


def compact_rays_dev(state, alive_bound, n_total, n_step_cap, max_steps, rays_alive, out_alive, out_state, workspace):
    _i32(rays_alive, 'rays_alive'); _i32(out_alive, 'out_alive'); _i32(out_state, 'out_state'); _i32(state, 'state')
    capi.check(capi.lib.ngp_compact_rays_dev(capi.ptr(state), alive_bound, n_total, n_step_cap, max_steps, capi.ptr(rays_alive), capi.ptr(out_alive),
                                             capi.ptr(out_state), capi.ptr(workspace), capi.stream()))


def ray_sample_ts(xyzs, rays_o, rays_d, rays, M, N, bound, ts):
    """extension (include/ngp_hip.h, ngp_ray_sample_ts): the t of every sample the marcher wrote, recovered from xyzs.  ctypes-only, like the
    geometry and feature compositors."""
    floats = ((xyzs, 'xyzs'), (rays_o, 'rays_o'), (rays_d, 'rays_d'), (ts, 'ts'))
    fn = capi.lib.ngp_ray_sample_ts_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_ray_sample_ts)
    _i32(rays, 'rays')
    capi.check(fn(capi.ptr(xyzs), capi.ptr(rays_o), capi.ptr(rays_d), capi.ptr(rays), M, N, float(bound), capi.ptr(ts), capi.stream()))


def ray_points_forward(rays_o, rays_d, ts, rays, M, N, bound, xyzs, dirs):
    """extension (ngp_ray_points_forward): xyzs = clamp(o + t d), dirs = d for the samples the rays own, zeros elsewhere"""
    floats = ((rays_o, 'rays_o'), (rays_d, 'rays_d'), (ts, 'ts'), (xyzs, 'xyzs'), (dirs, 'dirs'))
    fn = capi.lib.ngp_ray_points_forward_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_ray_points_forward)
    _i32(rays, 'rays')
    capi.check(fn(capi.ptr(rays_o), capi.ptr(rays_d), capi.ptr(ts), capi.ptr(rays), M, N, float(bound), capi.ptr(xyzs), capi.ptr(dirs), capi.stream()))


def ray_points_backward(grad_xyzs, grad_dirs, grad_sh16, xyzs, ts, rays_d, rays, M, N, bound, grad_rays_o, grad_rays_d):
    """extension (ngp_ray_points_backward): per-sample gradients -> per-ray gradients.  grad_dirs [M,3] and grad_sh16 [M,32] fp16 (fp32 calls
    only) may be None."""
    floats = ((grad_xyzs, 'grad_xyzs'), (grad_dirs, 'grad_dirs'), (xyzs, 'xyzs'), (ts, 'ts'), (rays_d, 'rays_d'), (grad_rays_o, 'grad_rays_o'),
              (grad_rays_d, 'grad_rays_d'))
    floats = tuple(p for p in floats if p[0] is not None)
    _i32(rays, 'rays')
    if _f64(floats):
        if grad_sh16 is not None:
            raise RuntimeError("ray_points_backward: grad_sh16 belongs to the float32 call (the fused path's fp16 colour-net input gradient)")
        capi.check(capi.lib.ngp_ray_points_backward_f64(capi.ptr(grad_xyzs), capi.ptr(grad_dirs), capi.ptr(xyzs), capi.ptr(ts), capi.ptr(rays_d),
                                                        capi.ptr(rays), M, N, float(bound), capi.ptr(grad_rays_o), capi.ptr(grad_rays_d), capi.stream()))
        return
    _f32_call(floats, None)
    if grad_sh16 is not None:
        capi.dense(grad_sh16, 'grad_sh16')
        if grad_sh16.dtype != torch.float16 or grad_sh16.dim() != 2 or tuple(grad_sh16.shape) != (M, 32):
            raise RuntimeError(f"grad_sh16 must be a float16 [M,32] tensor with M = {M} (got {grad_sh16.dtype}, {tuple(grad_sh16.shape)})")
    capi.check(capi.lib.ngp_ray_points_backward(capi.ptr(grad_xyzs), capi.ptr(grad_dirs), capi.ptr(grad_sh16), capi.ptr(xyzs), capi.ptr(ts),
                                                capi.ptr(rays_d), capi.ptr(rays), M, N, float(bound), capi.ptr(grad_rays_o), capi.ptr(grad_rays_d),
                                                capi.stream()))


def sdf_sigmas_forward(sdf, normals, dirs, deltas, inv_s, M, cos_anneal, sigmas):
    """extension (include/ngp_hip.h, ngp_sdf_sigmas_forward): NeuS's section opacity as the density that reproduces it.  ctypes-only, like the
    geometry and feature compositors."""
    floats = ((sdf, 'sdf'), (normals, 'normals'), (dirs, 'dirs'), (deltas, 'deltas'), (inv_s, 'inv_s'), (sigmas, 'sigmas'))
    fn = capi.lib.ngp_sdf_sigmas_forward_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_sdf_sigmas_forward)
    capi.check(fn(capi.ptr(sdf), capi.ptr(normals), capi.ptr(dirs), capi.ptr(deltas), capi.ptr(inv_s), M, float(cos_anneal), capi.ptr(sigmas),
                  capi.stream()))


def sdf_sigmas_backward(grad_sigmas, sdf, normals, dirs, deltas, inv_s, M, cos_anneal, grad_sdf, grad_normals, grad_dirs, grad_inv_s):
    """extension (ngp_sdf_sigmas_backward): every row of grad_sdf / grad_normals / grad_dirs (None: not wanted) and grad_inv_s [1], the latter
    through a fixed-order sum over a workspace allocated here (M == 0: nothing is launched, grad_inv_s stays as the caller made it)"""
    floats = tuple(p for p in ((grad_sigmas, 'grad_sigmas'), (sdf, 'sdf'), (normals, 'normals'), (dirs, 'dirs'), (deltas, 'deltas'), (inv_s, 'inv_s'),
                               (grad_sdf, 'grad_sdf'), (grad_normals, 'grad_normals'), (grad_dirs, 'grad_dirs'), (grad_inv_s, 'grad_inv_s'))
                   if p[0] is not None)
    fn = capi.lib.ngp_sdf_sigmas_backward_f64 if _f64(floats) else _f32_call(floats, capi.lib.ngp_sdf_sigmas_backward)
    n = int(capi.lib.ngp_sdf_sigmas_workspace_bytes(M))
    ws = torch.empty(n, dtype=torch.uint8, device=sdf.device) if n else None
    capi.check(fn(capi.ptr(grad_sigmas), capi.ptr(sdf), capi.ptr(normals), capi.ptr(dirs), capi.ptr(deltas), capi.ptr(inv_s), M, float(cos_anneal),
                  capi.ptr(grad_sdf), capi.ptr(grad_normals), capi.ptr(grad_dirs), capi.ptr(grad_inv_s), capi.ptr(ws), n, capi.stream()))


def _counts(t, name, words):
    capi.dense(t, name)
    if t.dtype != torch.int32 or t.numel() < words:
        raise RuntimeError(f"{name} must be an int tensor of at least {words} element(s)")
    return t


def _volume_dims(volume):
    _f32(volume, 'volume')
    if volume.dim() != 3:
        raise RuntimeError(f"volume must be [nz, ny, nx] (got {tuple(volume.shape)})")
    nz, ny, nx = volume.shape
    return nx, ny, nz


def surface_nets_workspace(volume):
    """the workspace ngp_surface_nets_count and _emit share for this volume (uint8 tensor)"""
    nx, ny, nz = _volume_dims(volume)
    n = int(capi.lib.ngp_surface_nets_workspace_bytes(nx, ny, nz)) if nx * ny * nz < (1 << 31) else 0   # (ctypes would wrap a larger extent)
    if n == 0:
        raise RuntimeError(f"surface_nets: every dimension must be at least 2 and nx * ny * nz below 2^31 (got {nx} x {ny} x {nz})")
    return torch.empty(n, dtype=torch.uint8, device=volume.device)


def surface_nets_count(volume, level, inside_below, workspace, counts):
    """extension (include/ngp_hip.h, ngp_surface_nets_count): counts[0] = vertices, counts[1] = triangles (int32 [2]; -1: does not fit)"""
    nx, ny, nz = _volume_dims(volume)
    capi.dense(workspace, 'workspace'); _counts(counts, 'counts', 2)
    capi.check(capi.lib.ngp_surface_nets_count(capi.ptr(volume), nx, ny, nz, float(level), int(bool(inside_below)), capi.ptr(workspace),
                                               capi.ptr(counts), capi.stream()))


def surface_nets_emit(volume, level, inside_below, origin, spacing, workspace, vertices, faces):
    """extension (ngp_surface_nets_emit), after surface_nets_count with the same volume, level, sense and workspace: vertices [v_cap,3] fp32,
    faces [f_cap,3] int32; raises ('truncated') when a capacity is below its count -- nothing is written past the buffers"""
    nx, ny, nz = _volume_dims(volume)
    _f32(vertices, 'vertices'); _i32(faces, 'faces'); capi.dense(workspace, 'workspace')
    if vertices.dim() != 2 or vertices.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f"surface_nets: expected vertices [V,3] and faces [F,3] (got {tuple(vertices.shape)}, {tuple(faces.shape)})")
    (ox, oy, oz), (hx, hy, hz) = (float(v) for v in origin), (float(v) for v in spacing)
    capi.check(capi.lib.ngp_surface_nets_emit(capi.ptr(volume), nx, ny, nz, float(level), int(bool(inside_below)), ox, oy, oz, hx, hy, hz,
                                              capi.ptr(workspace), capi.ptr(vertices), vertices.shape[0], capi.ptr(faces), faces.shape[0],
                                              capi.stream()))


def lattice_points(origin, spacing, nx, ny, z0, z1, bitfield, bound, C, H, dilate, points, index, count):
    """extension (ngp_lattice_points): the lattice points of the z-slab [z0, z1) near occupied space, compacted in lattice order; points
    [capacity,3] fp32, index [capacity] int32, count int32 [1] = K (the full count)"""
    _f32(points, 'points'); _i32(index, 'index'); _counts(count, 'count', 1)
    if bitfield is not None:
        capi.dense(bitfield, 'bitfield')
        if bitfield.dtype != torch.uint8 or bitfield.numel() * 8 < C * H ** 3:
            raise RuntimeError(f"bitfield must be a uint8 tensor of at least {C} * {H}^3 / 8 bytes")
    if points.dim() != 2 or points.shape[1] != 3 or index.numel() < points.shape[0]:
        raise RuntimeError(f"lattice_points: expected points [capacity,3] and index [capacity] (got {tuple(points.shape)}, {tuple(index.shape)})")
    n = int(capi.lib.ngp_lattice_points_workspace_bytes(nx, ny, max(z1 - z0, 0)))
    ws = torch.empty(max(n, 4), dtype=torch.uint8, device=points.device)
    (ox, oy, oz), (hx, hy, hz) = (float(v) for v in origin), (float(v) for v in spacing)
    capi.check(capi.lib.ngp_lattice_points(ox, oy, oz, hx, hy, hz, nx, ny, z0, z1, capi.ptr(bitfield), float(bound), C, H, dilate, capi.ptr(ws),
                                           capi.ptr(points), capi.ptr(index), capi.ptr(count), points.shape[0], capi.stream()))


def _accept_half(fn):
    """the reference dispatches its raymarching entry points on the tensor dtype (AT_DISPATCH_FLOATING_TYPES_AND_HALF, raymarching.cu:486);
    its own wrappers always hand over fp32 (custom_fwd(cast_inputs=float32)), so fp16 is unreachable from them.  For direct `_backend`
    callers: fp16 tensors are computed through fp32 copies of the same kernels and every floating tensor argument is copied back
    (outputs are caller-allocated arguments), i.e. fp32 arithmetic rounded once to fp16."""
    import functools

    @functools.wraps(fn)
    def call(*args):
        if not any(torch.is_tensor(a) and a.dtype == torch.float16 for a in args):
            return fn(*args)
        up = [a.float() if torch.is_tensor(a) and a.dtype == torch.float16 else a for a in args]
        out = fn(*up)
        for a, u in zip(args, up):
            if torch.is_tensor(a) and a.dtype == torch.float16:
                a.copy_(u)
        return out
    return call


near_far_from_aabb, sph_from_ray, packbits = _accept_half(near_far_from_aabb), _accept_half(sph_from_ray), _accept_half(packbits)
march_rays_train, march_rays, composite_rays = _accept_half(march_rays_train), _accept_half(march_rays), _accept_half(composite_rays)
composite_rays_train_forward = _accept_half(composite_rays_train_forward)
composite_rays_train_backward = _accept_half(composite_rays_train_backward)

_backend = types.SimpleNamespace(
    march_rays_dev=march_rays_dev, composite_rays_dev=composite_rays_dev, compact_rays_dev=compact_rays_dev,
    coarse_occupancy=coarse_occupancy, cull_rays=cull_rays,
    near_far_from_aabb=near_far_from_aabb, sph_from_ray=sph_from_ray, morton3D=morton3D, morton3D_invert=morton3D_invert,
    packbits=packbits, packbits_capped=packbits_capped, density_grid_update=density_grid_update,
    density_grid_update_workspace_bytes=density_grid_update_workspace_bytes, march_rays_train=march_rays_train, composite_rays_train_forward=composite_rays_train_forward,
    composite_rays_train_backward=composite_rays_train_backward, march_rays=march_rays, march_rays_ex=march_rays_ex,
    composite_rays=composite_rays,
    compact_rays=compact_rays)

__all__ = ['_backend']
