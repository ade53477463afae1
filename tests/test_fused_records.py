"""Host side of the fused training step (no GPU): the named records of fused.py and the deposit hand-off of optim.py.

The records replaced positional tuples, so the field ORDER is part of the contract (external callers may still unpack them); the deposit
functions replaced assignments to four marks on the torch Parameter that tests/test_ddp_gloo.py, tests/test_gpu_graph.py and
tests/test_gpu_table_adam.py still read and write directly, so the marks they leave are pinned here on a bare Parameter."""
import types

import numpy as np
import pytest
import torch


def test_network_cfg_is_a_named_record_in_the_positional_order():
    import fused
    from nerf.network_ff import NeRFNetwork
    m = NeRFNetwork(bound=1, cuda_ray=True)
    enc, sn, cn = m.encoder, m.sigma_net, m.color_net
    cfg = fused.network_cfg(enc, sn, cn, m.bound, True)
    assert cfg._fields == ('bound', 'L', 'S', 'H', 'gridtype', 'align', 'interp', 'nl_sigma', 'nl_color', 'training')
    positional = (float(m.bound), int(enc.num_levels), float(np.log2(enc.per_level_scale)), int(enc.base_resolution), int(enc.gridtype_id),
                  int(bool(enc.align_corners)), int(enc.interp_id), int(sn.num_layers), int(cn.num_layers), True)
    assert tuple(cfg) == positional
    (bound, L, S, H, gridtype, align, interp, nl_sigma, nl_color, training) = cfg          # still unpacks
    assert (cfg.bound, cfg.L, cfg.S, cfg.H, cfg.gridtype, cfg.align, cfg.interp, cfg.nl_sigma, cfg.nl_color, cfg.training) == positional
    assert (cfg.bound, cfg.L, cfg.H, cfg.nl_sigma, cfg.nl_color) == (1.0, 16, 16, 2, 3) and [type(v) for v in cfg] == [type(v) for v in positional]
    assert fused.network_cfg(enc, sn, cn, m.bound, False).training is False
    with pytest.raises(AttributeError):
        cfg.L = 8                                                                           # frozen
    # the other records of the step, in the order their producers fill them
    assert fused.RenderCfg._fields == ('cascade', 'grid_size', 'min_near', 'capacity', 'perturb', 'dt_gamma', 'max_steps', 'T_thresh',
                                       'density_scale', 'bg_scalar')
    assert fused.Marched._fields == ('xyzs', 'dirs', 'deltas', 'rays', 'nears', 'fars', 'ws')
    assert fused.Bufs._fields == ('emb16', 'ws16', 'wc16', 'g_emb', 'g_ws', 'g_wc')
    assert fused.Saved._fields.index('rays') == 12 and len(fused.Saved._fields) == 17
    bg_t, rcfg = fused._render_cfg(m, 8192, 1, True, 0, 1024, 1e-4)
    assert bg_t is None and rcfg.capacity == 8192 and rcfg.perturb is True and rcfg.bg_scalar == 1.0 and rcfg.density_scale == float(m.density_scale)


def test_deposit_hand_off_on_a_bare_parameter():
    """clean -> overwritten -> stale -> clean, as tests/test_ddp_gloo.py::test_kept_deposit_buffer_protocol_on_the_host finds the marks
    around step(); the table-sweep announcement; the replay's restatement; the consumer's refusal"""
    import optim
    p = torch.nn.Parameter(torch.randn(64, 2) * 0.1)
    p._ngp_grad16 = torch.zeros(64, 2, dtype=torch.half)

    def marks():
        return bool(getattr(p, '_ngp_deposit_overwritten', False)), bool(getattr(p, '_ngp_grad16_stale', False))
    consumer = types.SimpleNamespace(flat_params=[p])
    assert marks() == (False, False)                                  # clean
    optim.clean_deposits([p])                                         # an adding producer's request on a clean buffer: nothing to do
    p._ngp_grad16.add_(0.25)                                          # added-into: no mark
    assert marks() == (False, False)
    optim._consumed(p, kept=False)                                    # step(): the kernel zeroed it
    assert marks() == (False, False)
    p._ngp_grad16.fill_(0.5)
    optim.announce_overwrite(p)                                       # overwritten this step
    assert marks() == (True, False) and not getattr(p, '_ngp_table_adam_done', False)
    optim.NGPAdam._refuse_stale_deposits(consumer, 'step')            # (announced: a consumer accepts it)
    optim._consumed(p, kept=True)                                     # step() / apply(zero=False): kept, stale from here on
    assert marks() == (False, True) and float(p._ngp_grad16.float().min()) == 0.5
    with pytest.raises(RuntimeError, match='stale'):                  # a consumer must not take the previous step's gradient again
        optim.NGPAdam._refuse_stale_deposits(consumer, 'all_reduce')
    optim.announce_overwrite(p)                                       # stale -> overwritten: the next overwriting producer
    assert marks() == (True, True)
    optim.NGPAdam._refuse_stale_deposits(consumer, 'step')
    optim._consumed(p, kept=True)
    optim.NGPAdam.clean_deposits([p])                                 # stale -> clean (the spelling of graph.py and the tests)
    assert marks() == (False, False) and float(p._ngp_grad16.float().abs().max()) == 0.0
    optim.announce_overwrite(p)
    optim._consumed(p, kept=False)                                    # apply(zero=True): clean, whatever was announced
    assert marks() == (False, False)
    optim.replayed_kept_deposits([p, torch.nn.Parameter(torch.zeros(3))])   # after a graph replay; a parameter without a buffer is left alone
    assert marks() == (False, True)
    optim.clean_deposits([p])
    # the table-sweep announcement carries the dense-level prefix
    optim.announce_overwrite(p, table_adam_prefix=37)
    assert marks() == (True, False) and p._ngp_table_adam_done is True and p._ngp_table_adam_prefix == 37
    # the shadow half: a write from outside bumps the version, the resync refreshes the fp16 copy
    p._ngp_fp16 = torch.zeros(64, 2, dtype=torch.half)
    optim.resync_stale_shadows([p])
    assert torch.equal(p._ngp_fp16, p.detach().half()) and p._ngp_version == p._version
    with torch.no_grad():
        p.mul_(2.0)
    assert p._ngp_version != p._version
    optim.resync_stale_shadows([p])
    assert torch.equal(p._ngp_fp16, p.detach().half()) and p._ngp_version == p._version
