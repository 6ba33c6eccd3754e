"""Diagnostic (not shipped): build the library with -DMT_MEL_DIAG and print the per-phase wall time of wave 0 of every workgroup
of mel_kernel<false>, one forward's worth of chunks: python tools/mel_diag.py [B]"""
import ctypes as C, glob, os, subprocess, sys, tempfile
import numpy as np, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
csrc = os.path.join(ROOT, "music-transcription_amd", "csrc")
so = os.path.join(tempfile.mkdtemp(), "libmt_mel_diag.so")
subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-DMT_MEL_DIAG", f"-I{ROOT}/include", "-shared",
                       *sorted(glob.glob(os.path.join(csrc, "*.hip"))), "-o", so])
label = "mel_kernel<false>"
B = int(sys.argv[1]) if len(sys.argv) > 1 else 128
lib = C.CDLL(so)
vp = C.c_void_p
class Desc(C.Structure): _fields_ = [(n, C.c_int) for n in ("sr", "hop", "n_mels", "ell_rows")]
lib.mt_mel_plan_bytes.restype = C.c_size_t
lib.mt_mel_plan_init.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, C.c_int, C.POINTER(Desc), vp]
lib.mt_mel_db_f32.argtypes = [vp, C.POINTER(Desc), vp, C.c_int, C.c_int, vp, vp, C.c_int, vp]
lib.mt_mel_diag_read.argtypes = [vp]
N = 480000
torch.manual_seed(0)
wave = (torch.randn(B, N, device="cuda") * 0.1).contiguous()
plan = torch.empty(lib.mt_mel_plan_bytes(320), dtype=torch.uint8, device="cuda")
d = Desc(); st = torch.cuda.current_stream().cuda_stream
assert lib.mt_mel_plan_init(plan.data_ptr(), plan.numel(), 16000, 512, 320, d, st) == 0
T = 1 + N // 512
mel = torch.empty(B, 320, T, device="cuda"); cm = torch.empty(B, device="cuda")
NL = 5
for _ in range(2):
    assert lib.mt_mel_db_f32(plan.data_ptr(), d, wave.data_ptr(), B, N, mel.data_ptr(), cm.data_ptr(), 0, st) == 0
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(NL):
    assert lib.mt_mel_db_f32(plan.data_ptr(), d, wave.data_ptr(), B, N, mel.data_ptr(), cm.data_ptr(), 0, st) == 0
e1.record(); torch.cuda.synchronize()
out = np.zeros((1024, 12), dtype=np.uint64)
lib.mt_mel_diag_read(out.ctypes.data)
tiles = B * ((T + 31) // 32)
nblk = min(tiles, 256)
x = out[:nblk].astype(np.float64) * 10.0      # ns, last launch, wave 0 of each block, summed over the block's tiles
tot = x[:, :9].sum(1).mean()
names = ["wait at loop top", "window (load wait)", "fft A", "twiddle", "transpose", "fft B", "split+power", "mel+dB", "tile store"]
print(f"== {label}: B={B} T={T} tiles={tiles} blocks={nblk}; diag-build launch {e0.elapsed_time(e1) / NL * 1e3:.1f} us (incl. memset)")
for i, n in enumerate(names):
    print(f"{n:22s} {x[:, i].mean() / 1e3:8.1f} us per block  {100 * x[:, i].mean() / tot:5.1f} %")
print(f"{'sum':22s} {tot / 1e3:8.1f} us per block; checksum {float(mel.double().sum()):.6e} cmax {float(cm.view(torch.int32).double().sum()):.0f}")
