"""The UV-net entry points of the C ABI called through ctypes on the tensors of a tests/uvnet_ref.Net, so that NULL pointers reach the
kernels and every output buffer is longer than what the kernel owns: texgs_uv_pack + texgs_uv_taylor_packed, texgs_uv_backward."""
import ctypes as C

import torch

import uvnet_ref as R

SENTINEL = -7.5
GUARD = 64                  # floats on either side of every backward output


def _net_struct(net, emb, dev):
    from texgs import _lib
    f = lambda t: None if t is None else t.detach().to(device=dev, dtype=torch.float32).contiguous()
    W, b = [f(w) for w in net.W], [f(x) for x in net.b]
    both = net.off is not None and net.scale is not None
    keep = [W[0], b[0], W[1], b[1], f(emb), W[2], b[2], W[3], b[3], W[4], b[4], f(net.off) if both else None, f(net.scale) if both else None]
    return _lib.UVNetStruct(*[_lib.ptr(t) for t in keep], R.HIDDEN), keep


def forward(net, emb, xyz, precision, pad_rows=32, dev="cuda:0"):
    """-> (uvs [N + pad_rows, 3], J [N + pad_rows, 9]) on the host: the whole buffers, pre-filled with SENTINEL."""
    from texgs import _lib
    lib = _lib.load()
    dev = torch.device(dev)
    st, keep = _net_struct(net, emb, dev)
    prec = _lib.UV_PRECISION[precision]
    x = xyz.to(device=dev, dtype=torch.float32).contiguous()
    n = x.shape[0]
    packed = torch.empty(lib.texgs_uv_packed_bytes(prec), dtype=torch.uint8, device=dev)
    uvs = torch.full((n + pad_rows, 3), SENTINEL, dtype=torch.float32, device=dev)
    J = torch.full((n + pad_rows, 9), SENTINEL, dtype=torch.float32, device=dev)
    with _lib.on(dev) as stream:
        _lib.call(lib.texgs_uv_pack, C.byref(st), prec, packed.data_ptr(), stream)
        _lib.call(lib.texgs_uv_taylor_packed, C.byref(st), prec, packed.data_ptr(), x.data_ptr(), n, uvs.data_ptr(), J.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    del keep
    return uvs.cpu(), J.cpu()


def backward(net, emb, xyz, g, precision, null_outputs=(), dev="cuda:0"):
    """-> ({name: gradient on the host, or None for a name in null_outputs}, guards_untouched).  Every output lies between two guards
    of GUARD sentinel words; an output passed as NULL is not allocated."""
    from texgs import _lib
    lib = _lib.load()
    dev = torch.device(dev)
    st, keep = _net_struct(net, emb, dev)
    x = xyz.to(device=dev, dtype=torch.float32).contiguous()
    gg = g.to(device=dev, dtype=torch.float32).contiguous()
    n = x.shape[0]
    bufs, ptrs = {}, []
    for name in R.NAMES:
        if name in null_outputs:
            ptrs.append(None)
            continue
        numel = 1
        for s in R.SHAPES[name]:
            numel *= s
        bufs[name] = torch.full((numel + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
        ptrs.append(bufs[name].data_ptr() + 4 * GUARD)
    gr = _lib.UVNetGradStruct(*ptrs)
    with _lib.on(dev) as stream:
        temp = torch.empty(lib.texgs_uv_backward_temp_bytes(n), dtype=torch.uint8, device=dev)
        _lib.call(lib.texgs_uv_backward, C.byref(st), _lib.UV_PRECISION[precision], x.data_ptr(), gg.data_ptr(), n, C.byref(gr), temp.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    del keep
    out, clean = {}, True
    for name in R.NAMES:
        if name in null_outputs:
            out[name] = None
            continue
        h = bufs[name].cpu()
        clean &= bool((h[:GUARD] == SENTINEL).all()) and bool((h[-GUARD:] == SENTINEL).all())
        out[name] = h[GUARD:-GUARD].reshape(R.SHAPES[name]).clone()
    return out, clean
