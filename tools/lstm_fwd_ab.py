"""Diagnostic (not shipped): time the in-tree recurrences -- forward in train mode, inference with f32 gx, inference with f16 gx, the fused-projection
forward, and the backward (H <= 512) -- and print a checksum of what each writes, so that builds (MT_LSTM_AB_LIB=<variant .so>) and knobs (MT_LSTM_C16)
can be compared launch for launch.   python tools/lstm_fwd_ab.py [B T H]"""
import ctypes as C, os, sys
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = C.CDLL(os.environ.get("MT_LSTM_AB_LIB") or os.path.join(ROOT, "music-transcription_amd", "libmt_hip.so"))
B, T, H = (int(v) for v in (sys.argv[1:4] if len(sys.argv) >= 4 else (16, 937, 512)))
vp, sz, ci = C.c_void_p, C.c_size_t, C.c_int
for f in ("mt_lstm_gx_bytes", "mt_lstm_hx_bytes", "mt_lstm_cx_bytes", "mt_lstm_sync_bytes", "mt_lstm_dgx_bytes", "mt_lstm_bwd_part_bytes"):
    getattr(lib, f).restype = sz
torch.manual_seed(0)
gx0 = torch.randn(lib.mt_lstm_gx_bytes(B, T, H) // 4, device="cuda") * 0.5
gx16 = gx0.half()
whh = ((torch.rand(2, 4 * H, H, device="cuda") * 2 - 1) / np.sqrt(H)).contiguous()
wihx = ((torch.rand(2, 4 * H, 2 * H, device="cuda") * 2 - 1) / np.sqrt(2 * H)).contiguous()
bias = torch.randn(2, 4 * H, device="cuda") * 0.1
hx = torch.empty(lib.mt_lstm_hx_bytes(B, T, H) // 4, device="cuda")
hx2 = torch.empty_like(hx)
cx = torch.empty(lib.mt_lstm_cx_bytes(B, T, H) // 4, device="cuda")
dh = torch.randn(cx.numel(), device="cuda") * 0.1
sync = torch.empty(lib.mt_lstm_sync_bytes(B, H), dtype=torch.uint8, device="cuda")
lib.mt_lstm_bidir_fwd_train.argtypes = [vp, vp, vp, vp, vp, sz, ci, ci, ci, vp]
lib.mt_lstm_bidir_fwd.argtypes = [vp, vp, vp, vp, sz, ci, ci, ci, vp]
lib.mt_lstm_bidir_fwd_ex.argtypes = [vp, vp, vp, vp, sz, ci, ci, ci, ci, vp]
lib.mt_lstm_bidir_fwd_xproj.argtypes = [vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, vp]
lib.mt_lstm_bidir_bwd.argtypes = [vp, vp, vp, vp, vp, vp, sz, vp, sz, ci, ci, ci, vp]
st = torch.cuda.current_stream().cuda_stream
env = {k: os.path.basename(v) for k, v in os.environ.items() if k.startswith("MT_LSTM")}
isum = lambda x: int(x.view(torch.int32).to(torch.int64).sum().item())
modes = ["train", "infer", "g16"] + (["xproj", "bwd"] if H <= 512 else [])
gates = None
for mode in modes:
    if mode == "bwd":               # gates and cx as the train-mode forward above left them
        dgx = torch.empty(lib.mt_lstm_dgx_bytes(B, T, H), dtype=torch.uint8, device="cuda")
        part = torch.empty(lib.mt_lstm_bwd_part_bytes(B, T, H), dtype=torch.uint8, device="cuda")
    ts = []
    for it in range(8):
        gx = gx0.clone()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        if mode == "train":
            rc = lib.mt_lstm_bidir_fwd_train(gx.data_ptr(), whh.data_ptr(), hx.data_ptr(), cx.data_ptr(), sync.data_ptr(), sync.numel(), B, T, H, st)
        elif mode == "infer":
            rc = lib.mt_lstm_bidir_fwd(gx.data_ptr(), whh.data_ptr(), hx.data_ptr(), sync.data_ptr(), sync.numel(), B, T, H, st)
        elif mode == "g16":
            rc = lib.mt_lstm_bidir_fwd_ex(gx16.data_ptr(), whh.data_ptr(), hx2.data_ptr(), sync.data_ptr(), sync.numel(), B, T, H, 0x10, st)
        elif mode == "xproj":       # input: the hx of the "infer" mode
            rc = lib.mt_lstm_bidir_fwd_xproj(hx.data_ptr(), wihx.data_ptr(), bias.data_ptr(), whh.data_ptr(), hx2.data_ptr(), sync.data_ptr(), sync.numel(), B, T, H, st)
        else:
            rc = lib.mt_lstm_bidir_bwd(gates.data_ptr(), cx.data_ptr(), dh.data_ptr(), whh.data_ptr(), dgx.data_ptr(), part.data_ptr(), part.numel(),
                                       sync.data_ptr(), sync.numel(), B, T, H, st)
        e1.record(); torch.cuda.synchronize()
        assert rc == 0 and int(sync[:4].view(torch.int32).item()) == 0, (mode, rc, hex(int(sync[:4].view(torch.int32).item())))
        ts.append(e0.elapsed_time(e1))
    if mode == "train":
        gates = gx
    chk = {"train": lambda: isum(hx) + isum(cx) + isum(gx), "infer": lambda: isum(hx), "g16": lambda: isum(hx2), "xproj": lambda: isum(hx2),
           "bwd": lambda: isum(dgx)}[mode]()
    print(f"{env}  {mode} B={B} T={T} H={H}: min {min(ts):.3f} ms  median {sorted(ts)[len(ts) // 2]:.3f} ms (incl. the poison fill) = {1e3 * min(ts) / T:.2f} us/step  checksum {chk}")
