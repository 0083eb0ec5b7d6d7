"""tools/so3_f64_time.py -- what the float64 regime of the SO(3) conv layers costs on the MI355X (profiles/so3_float64.txt).

    python tools/so3_f64_time.py [--out profiles/so3_float64.txt] [--reps 3]

  1. the three forms of the float64 GEMM (csrc/so3_f64.hip, v_mfma_f64_16x16x4_f64) at 512 x 3072 x 245760 -- one cloud of the 128 -> 512
     layer: Y = W X, dX = W^T gY, dW = gY X^T: time (device events, median of --reps after a warm-up call), achieved TFLOP/s
     (2 M N K over the time) and the shader clock the device reports;
  2. forward and forward + backward of the 64 -> 128 and 128 -> 512 inter conv layers of the benchmark backbone (synth_clouds.backbone_layers,
     NN = 64, 60 anchors, permute_modes = 1) at 2 x 4096 points in float64, beside the SAME layer in float32 on the same inputs with the dense
     product off (vgtk.so3conv.functional.DENSE_MODE = 'off', what EAP_DENSE=off selects: the fp32 list kernels), and the peak of allocated
     memory of each run.

A measurement path that finds no GPU fails."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'equi-articulated-pose_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'so3_float64.txt'))
    ap.add_argument('--reps', type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('so3_f64_time: needs the GPU (a timing taken elsewhere says nothing)')
    import synth_clouds
    import vgtk.so3conv as sptk
    import vgtk.so3conv.functional as L
    import vgtk.spconv as zptk
    from vgtk import _hip
    dev = torch.device('cuda:0')
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms), max(ms)

    props = torch.cuda.get_device_properties(0)
    try:        # hipDeviceAttributeClockRate (5): the peak shader clock in kHz
        import ctypes
        khz = ctypes.c_int(0)
        rc = ctypes.CDLL('libamdhip64.so').hipDeviceGetAttribute(ctypes.byref(khz), 5, 0)
        clock = f'{khz.value / 1e3:.0f} MHz' if rc == 0 else f'not reported (hip error {rc})'
    except Exception as e:
        clock = f'not reported ({e})'
    say(f'device: {props.name}, {props.multi_processor_count} CUs, peak shader clock (hipDeviceAttributeClockRate) {clock}')
    say(f'--reps {args.reps}: median [min .. max] of that many calls after one warm-up call, device events')
    say()
    say('1. float64 GEMM forms at O x CK x PA = 512 x 3072 x 245760 (one cloud of the 128 -> 512 layer)')
    O, CK, PA = 512, 3072, 245760
    gen = torch.Generator(device=dev).manual_seed(1)
    W = torch.randn(O, CK, dtype=torch.float64, device=dev, generator=gen)
    X = torch.randn(1, CK, PA, dtype=torch.float64, device=dev, generator=gen)
    gY = torch.randn(1, O, PA, dtype=torch.float64, device=dev, generator=gen)
    Y, dX, dW = torch.empty(1, O, PA, dtype=torch.float64, device=dev), torch.empty_like(X), torch.empty_like(W)
    flops = 2.0 * O * CK * PA
    for name, fn in (('Y  = W X      (M, N, K) = (512, 245760, 3072)  ', lambda: _hip.matmul(W, X, Y)),
                     ('dX = W^T gY   (M, N, K) = (3072, 245760, 512)  ', lambda: _hip.matmul(W.t(), gY, dX)),
                     ('dW = gY X^T   (M, N, K) = (512, 3072, 245760)  ', lambda: _hip.matmul_reduce(gY, X.transpose(1, 2), dW))):
        med, lo, hi = timed(fn)
        say(f'   {name} {med:8.1f} ms [{lo:.1f} .. {hi:.1f}]   {flops / med / 1e9:6.2f} TFLOP/s')
    try:
        clocks = subprocess.run(['rocm-smi', '--showclocks', '-d', '0'], capture_output=True, text=True, timeout=30).stdout
        for ln in clocks.splitlines():
            if 'sclk' in ln:
                say('   shader clock right after the calls (rocm-smi --showclocks): ' + ' '.join(ln.split()))
    except Exception as e:      # the tool is optional: the device property above stays
        say(f'   (rocm-smi not available: {e})')
    del X, gY, Y, dX, dW, W
    torch.cuda.empty_cache()

    say()
    say('2. inter conv layers at 2 x 4096 points, NN = 64, 60 anchors, permute_modes = 1 (synth_clouds.laptop_batch(0, 2, 4096))')
    say(f'   float64: the float64 regime, F64_X_BYTES_MAX = {L.F64_X_BYTES_MAX >> 30} GiB;  float32: the same layer and inputs, dense product off '
        f'(the fp32 list kernels)')
    B, P = 2, 4096
    xyz_np, _, pose_np = synth_clouds.laptop_batch(0, B, P)
    L.DENSE_MODE = 'off'
    for layer in (1, 2):
        c, o, r, s = synth_clouds.backbone_layers(P)[layer]
        torch.manual_seed(2913)
        conv32 = sptk.InterSO3PoseConv(c, o, 1, 1, r, s, 64, kanchor=60, permute_modes=1).to(dev)
        feats32 = torch.randn(B, c, P, 60, device=dev)
        gy32 = torch.randn(B, o, P, 60, device=dev)
        for dtype in (torch.float32, torch.float64):
            conv = conv32 if dtype == torch.float32 else sptk.InterSO3PoseConv(c, o, 1, 1, r, s, 64, kanchor=60, permute_modes=1).to(dev).double()
            if dtype == torch.float64:
                conv.load_state_dict({k: v.double() for k, v in conv32.state_dict().items()})
            xyz, pose = torch.from_numpy(xyz_np).to(dev).to(dtype), torch.from_numpy(pose_np).to(dev).to(dtype)
            feats, gy = feats32.to(dtype).requires_grad_(True), gy32.to(dtype)
            cloud = zptk.SphericalPointCloudPose(xyz, feats, None, pose)

            def fwd():
                with torch.no_grad():
                    return conv(cloud)[3].feats

            def both():
                y = conv(cloud)[3].feats
                torch.autograd.grad(y, [feats, conv.basic_conv.W], gy)

            for what, fn in (('forward           ', fwd), ('forward + backward', both)):
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                med, lo, hi = timed(fn)
                peak = torch.cuda.max_memory_allocated() / 2 ** 30
                say(f'   {c:3d} -> {o:3d}  {str(dtype)[6:]}  {what} {med:9.1f} ms [{lo:.1f} .. {hi:.1f}]   peak allocated {peak:6.2f} GiB')
            del conv, feats, gy, cloud
        del conv32, feats32, gy32
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
