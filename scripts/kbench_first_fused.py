"""Kernel-level timing of the fused first block's forward (k_c1b_fwd<4, 1>, conv_first.hip: conv + BatchNorm + sign -> int8 codes + pass nibbles) on nin_gc's
shape at batch 256 (3 -> 256 channels, 5x5, 32x32).

    python scripts/kbench_first_fused.py [LABEL:ENV=V,ENV=V ...]        (e.g. base: ko_mfma:MN_LIB_PATH=micronet_amd/lib/libmicronet_hip_komfma.so)

Every variant runs in a child process (the library is loaded once per process); torch events around 50 launches of mn_conv2d_first_bnact_fwd with act = 1.  The
line also carries a checksum of the codes and the mask bytes, so that a variant meant to compute the same thing shows that it does.  GPU only."""
import ctypes as C
import json
import os
import subprocess
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import torch
    from micronet_amd import _lib
    lib = _lib.get_lib()
    N, Cin, H, W, O, k = 256, 3, 32, 32, 256, 5
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn((N, Cin, H, W), device="cuda", generator=gen)
    w = torch.randn((O, Cin, k, k), device="cuda", generator=gen) * 0.1
    b = torch.randn(O, device="cuda", generator=gen) * 0.1
    # any plausible statistics do: the kernel's time does not depend on them
    save = torch.stack([torch.zeros(O, device="cuda"), torch.ones(O, device="cuda")]).contiguous()
    gamma = torch.randn(O, device="cuda", generator=gen) * 0.5 + 1
    beta = torch.randn(O, device="cuda", generator=gen) * 0.3
    codes = torch.zeros((N, O, H, W), dtype=torch.int8, device="cuda")
    mask4 = torch.zeros((N, O, H * W // 4), dtype=torch.uint8, device="cuda")
    g = _lib.ConvGeom(N, Cin, H, W, O, k, k, 1, 1, k // 2, k // 2, 1, 1, 1)
    p = lambda t: C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch():
        rc = lib.mn_conv2d_first_bnact_fwd(C.byref(g), p(x), p(w), p(b), p(save), p(gamma), p(beta), 1, 0, p(codes), p(mask4), s)
        if rc != 0:
            raise RuntimeError(lib.mn_last_error().decode())
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        launch()
    e1.record()
    torch.cuda.synchronize()
    crc = zlib.crc32(mask4.cpu().numpy().tobytes(), zlib.crc32(codes.cpu().numpy().tobytes()))
    print(json.dumps({"us": round(e0.elapsed_time(e1) * 1000 / 50, 1), "kernel": lib.mn_last_kernel().decode(), "crc32": "%08x" % crc}))


if __name__ == "__main__":
    if os.environ.get("_KB_CHILD"):
        run()
        sys.exit(0)
    variants = sys.argv[1:] or ["base:"]
    for v in variants:
        label, _, envs = v.partition(":")
        env = dict(os.environ, _KB_CHILD="1")
        for kv in filter(None, envs.split(",")):
            k, _, val = kv.partition("=")
            env[k] = val
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
        line = [l for l in r.stdout.splitlines() if l.startswith("{")]
        print(label, line[-1] if line else ("FAILED rc=%d " % r.returncode + r.stderr[-300:]), flush=True)
        if r.returncode != 0:          # a child that died on the GPU: nothing more is started on it
            sys.exit(1)
