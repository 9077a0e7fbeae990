"""What every analysis of the calls shares on the Python side, each written once: the way of an array to the device, the check of a
launch function's tensor arguments, its outputs and its scratch, and the check of an integer argument.  The per-segment analyses
(measure.py, patches.py, pitch.py; see segments.py) and the row analyses (neighbors.py, dtw.py, linkage.py, pca.py, embed.py) use
these and hold no copy of their own.  Shapes and ranges stay with the analysis that knows them: they are ValueErrors, raised there."""
import numpy as np

from . import _lib


def resident(a, device):
    """numpy (uploaded to `device`) or a tensor (a device tensor stays where it lies) -> a contiguous float32 device tensor.  A
    contiguous float32 device tensor is returned as it is: no copy, no launch."""
    import torch
    if torch.is_tensor(a):
        return a.to(dtype=torch.float32).contiguous() if a.is_cuda else a.to(device=device, dtype=torch.float32).contiguous()
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float32)).to(device)


def shape_of(a):
    """The shape of a tensor, or of what numpy takes as an array, as a tuple: what an entry point checks before it looks for a device."""
    import torch
    return tuple(a.shape) if torch.is_tensor(a) else np.shape(a)


def check_tensor(t, name, layout, dtype=None, shape=None, device=None, ndim=None):
    """WsegError, `name` and `layout` in words, unless `t` is what a launch function may hand to a kernel: a contiguous device tensor
    of `dtype` (None: float32) and, where given, of `ndim` dimensions, of `shape` and on `device`."""
    import torch
    dtype = torch.float32 if dtype is None else dtype
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dtype and t.is_contiguous() and (ndim is None or t.dim() == ndim)
            and (shape is None or tuple(t.shape) == tuple(shape)) and (device is None or t.device == device)):
        where = "" if device is None else f" on {device}"
        raise _lib.WsegError(f"{name} must be a contiguous {str(dtype)[6:]} device tensor {layout}{where} (no CPU path)")


def out_tensor(out, name, layout, dtype, shape, device):
    """An output argument: a new tensor of `dtype` and `shape` on `device` for None, else `out` itself, checked as check_tensor does."""
    import torch
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    check_tensor(out, name, layout, dtype, shape, device)
    return out


def new_scratch(nbytes, device):
    import torch
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


def check_int(x, name, lo, hi, words=None):
    """`x` as an int; ValueError unless it is an int or a numpy integer, no bool, in lo .. hi.  `words`: the caller's own wording of
    the range ("in 1 .. min(64, N - 1) = 7")."""
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)) or not lo <= int(x) <= hi:
        raise ValueError(f"{name} must be an integer {words or f'in {lo} .. {hi}'} (got {x!r})")
    return int(x)
