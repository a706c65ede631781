"""MI355X-native LightGCN propagation engine (drop-in for the reference's models/lightgcn.py path).

    engine   ctypes binding of liblgcn_engine.so (include/lgcn.h), CSR plan cache, autograd
    graph    host-side normalised-adjacency builder (main.py:282-336) + synthetic generators
    loss     bpr_loss_reg with the reference signature (main.py:366-402)
    train    bpr_step: one fused BPR training step that keeps the batch indices (main.py:495-525);
             bpr_epoch: a whole epoch of them fed by the sampler
    sampler  BprSampler: the negatives of a whole epoch in one launch (main.py:349-363)
    optim    Adam: torch.optim.Adam's default step, bit for bit, as one launch (main.py's optimizer)
    dist     multi-GPU propagation (row partition + per-layer RCCL all-gather; feature split)
"""
__version__ = "0.1.0"

import importlib as _importlib
import os as _os
import sys as _sys



def __getattr__(name):
    # `gcn_recommendation_amd.sampler` / `.optim` on first use: importing the package itself still
    # imports neither torch nor the engine
    if name in ("sampler", "optim"):
        return _importlib.import_module(f"{__name__}.{name}")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _raise_hw_queues():
    """Under torch.distributed (WORLD_SIZE > 1) RCCL's communicator streams share HIP's hardware
    queues with the exact schedule's eight streams (world-1 featsplit step 16.3 ms at 4 or 8
    queues per priority vs 13.1 ms at 16). HIP reads GPU_MAX_HW_QUEUES once, when its
    runtime initialises, so a `torchrun main.py` rank gets 16 here, at import, unless something
    already touched the GPU or the environment asks for more (bench.py does the same)."""
    try:
        if int(_os.environ.get("WORLD_SIZE", "1") or 1) <= 1:
            return
        q = int(_os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4)
    except ValueError:
        return
    torch = _sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        return
    if q < 16:
        _os.environ["GPU_MAX_HW_QUEUES"] = "16"


_raise_hw_queues()
