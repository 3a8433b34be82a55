"""Which HIP runtime calls on a non-blocking stream wait for the null stream?  A fill is queued on the null stream behind about 42 ms of spin
kernels; then, on a stream of torch's (non-blocking), a device-to-host copy into pageable memory by hipMemcpyAsync, one by hipMemcpy2DAsync
(what the relationship kernels' entries issue for a host result), hipMalloc and hipFree.  Prints how long each took on the host and which
values a copy saw (0: the fill had not run; 1: the call waited for the null stream).  DESIGN.md section 3 quotes the figures: they decide
what tests/test_gpu_handles.py can and cannot see of a launch on stream 0.  Needs an MI355X and torch; no part of the library is loaded."""
import ctypes as C
import time

import numpy as np
import torch

D2H = 2      # hipMemcpyDeviceToHost


def main():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipStreamSynchronize.argtypes = [C.c_void_p]
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    s = torch.cuda.Stream()
    st = C.c_void_p(s.cuda_stream)
    nr, nc = 700, 300
    x = torch.zeros(nr * nc, dtype=torch.float64, device="cuda")
    p = C.c_void_p()

    def case(name, op):
        x.zero_()
        torch.cuda.synchronize()
        for _ in range(20):
            torch.cuda._sleep(5_000_000)      # on the null stream
        x.fill_(1.0)                          # queued behind them
        t0 = time.perf_counter()
        seen = op()
        t1 = time.perf_counter()
        print("%s: %.2f ms on the host%s" % (name, 1e3 * (t1 - t0), "" if seen is None else ", saw %.1f" % seen), flush=True)
        torch.cuda.synchronize()

    def copy1d():
        h = np.full(nr * nc, -7.0)
        assert hip.hipMemcpyAsync(h.ctypes.data, x.data_ptr(), nr * nc * 8, D2H, st) == 0 and hip.hipStreamSynchronize(st) == 0
        return float(h[0])

    def copy2d():
        h = np.full((nr, nc + 5), -7.0)
        assert hip.hipMemcpy2DAsync(h.ctypes.data, (nc + 5) * 8, x.data_ptr(), nc * 8, nc * 8, nr, D2H, st) == 0 and hip.hipStreamSynchronize(st) == 0
        return float(h[0, 0])

    def malloc():
        assert hip.hipMalloc(C.byref(p), 1 << 20) == 0

    def free():
        assert hip.hipFree(p) == 0

    case("hipMemcpyAsync to pageable memory", copy1d)
    case("hipMemcpy2DAsync to pageable memory", copy2d)
    case("hipMalloc", malloc)
    case("hipFree", free)


if __name__ == "__main__":
    main()
