"""`train_detector` (mmdet/apis/train.py:33-128): wrap the model for data-parallel training, build
the optimizer and the runner, register the training hooks, run."""
import contextlib

import torch

from .. import _lib
from ..parallel import DataParallelModel
from ..runner import DistEvalHook, DistSamplerSeedHook, EpochBasedRunner, EvalHook, build_optimizer


def math_mode_of(cfg):
    """The library math mode a config asks for: 'bf16' when it carries mmdet's `fp16` key (mmdet/apis/train.py:94-98),
    else None (the current mode stays)."""
    return 'bf16' if cfg.get('fp16') is not None else None


@contextlib.contextmanager
def config_math_mode(cfg, logger=None):
    """Runs the body in the math mode of `cfg` (math_mode_of) and restores the previous mode on the way out.  Yields the
    mode set, or None when the config asks for none."""
    mode = math_mode_of(cfg)
    if mode is None:
        yield None
        return
    log = logger.info if hasattr(logger, 'info') else (logger or print)
    fp16 = cfg.get('fp16')
    loss_scale = fp16.get('loss_scale') if isinstance(fp16, dict) else fp16
    prev = _lib.get_math_mode()
    _lib.set_math_mode(mode)
    log(f"fp16 config: contractions run in math mode '{mode}' (bf16 products, fp32 accumulation); parameters, "
        f"activations and gradients stay fp32, so loss_scale={loss_scale!r} is accepted and not applied")
    try:
        yield mode
    finally:
        _lib.set_math_mode(prev)


def train_detector(model, data_loaders, cfg, distributed=False, validate=False, timestamp=None, meta=None,
                   logger=None, channels_last=True):
    with config_math_mode(cfg, logger):
        return _train_detector(model, data_loaders, cfg, distributed, validate, meta, logger, channels_last)


def _train_detector(model, data_loaders, cfg, distributed, validate, meta, logger, channels_last):
    data_loaders = data_loaders if isinstance(data_loaders, (list, tuple)) else [data_loaders]
    if torch.cuda.is_available():
        model = model.cuda()
        if channels_last:
            model = model.to(memory_format=torch.channels_last)
    # One process per GPU; the wrapper also is the gradient arena of a single process (bucket views as `p.grad` and as the
    # kernels' gradient sinks, parallel/reducer.py), so it is used on the device whether or not there are peers.
    if distributed or next(model.parameters()).is_cuda:
        model = DataParallelModel(model)
    optimizer = build_optimizer(model, cfg.optimizer)
    runner = EpochBasedRunner(model, optimizer=optimizer, work_dir=cfg.get('work_dir'), logger=logger, meta=meta)
    runner.register_training_hooks(cfg.lr_config, cfg.optimizer_config, cfg.get('checkpoint_config'),
                                   cfg.get('log_config'))
    if distributed:
        runner.register_hook(DistSamplerSeedHook())
    if validate:                                   # mmdet/apis/train.py:112-122
        from ..data import build_dataloader, build_dataset
        val = build_dataset(cfg.data.val, dict(test_mode=True))
        loader = build_dataloader(val, samples_per_gpu=1, workers_per_gpu=cfg.data.get('workers_per_gpu', 0),
                                  dist=distributed, shuffle=False)
        hook = DistEvalHook if distributed else EvalHook
        runner.register_hook(hook(loader, **dict(cfg.get('evaluation', {}))))
    if cfg.get('resume_from'):
        runner.resume(cfg.resume_from)
    elif cfg.get('load_from'):
        runner.load_checkpoint(cfg.load_from)
    runner.run(list(data_loaders), cfg.workflow, cfg.total_epochs)
    return runner
