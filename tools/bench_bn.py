"""Times the BatchNorm / pool passes at the shapes of the B = 256 step, and the detector taps folded into them against
the BN pass plus the tap pass they replace (forward and backward, fp32 and bf16 tensors)."""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from pitchextractor_amd import ops  # noqa: E402

dev = torch.device('cuda:0')
def timed(fn, n=6):
    ts=[]
    for r in range(n):
        a,b=torch.cuda.Event(enable_timing=True),torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        if r: ts.append(a.elapsed_time(b))
    return sorted(ts)[len(ts)//2]
if "--taps-only" not in sys.argv:
  for (F,C,pool) in [(80,64,1),(80,64,2),(40,128,1),(40,128,2),(20,192,2),(10,256,4)]:
    for a16 in (False, True):
        with ops.matmul_bf16(True,'bf16',act16=a16):
            dt = ops.act_dtype()
            x = torch.randn(256,192,F,C,device=dev).to(dt)
            dy = torch.randn(256,192,F//pool,C,device=dev).to(dt)
            g,b = torch.ones(C,device=dev), torch.zeros(C,device=dev)
            st = ops.bn_train_stats(x, g, b, torch.zeros(C,device=dev), torch.ones(C,device=dev))
            dg, db = torch.zeros(C,device=dev), torch.zeros(C,device=dev)
            dx = torch.empty_like(x)
            t_b = timed(lambda: ops.bn_act_pool_bwd(x, dy, st, dg, db, pool=pool, slope=0.01, dx=dx))
            y = torch.empty(256,192,F//pool,C,device=dev,dtype=dt)
            t_f = timed(lambda: ops.bn_act_pool_fwd(x, st, pool=pool, slope=0.01, out=y))
            esz = 2 if a16 else 4
            nb = x.numel()*esz; nd = dy.numel()*esz
            bytes_b = 2*(nb+nd) + nb      # two sweeps of x and dy, one write of dx
            bytes_f = nb + nd
            print(f"F={F} C={C} pool={pool} {'bf16' if a16 else 'fp32'}: bwd {t_b:.3f} ms = {bytes_b/t_b/1e9:.2f} TB/s   fwd {t_f:.3f} ms = {bytes_f/t_f/1e9:.2f} TB/s")
        del x, dy, dx, y

# detector taps: the fused pass against the BN pass followed by the tap pass (what FOLD_TAPS replaces)
for (F,C,tap_pool,coff) in [(80,64,40,0),(40,128,20,64),(20,192,10,192)]:
    for a16 in (False, True):
        dt = torch.bfloat16 if a16 else torch.float32
        x = torch.randn(256,192,F,C,device=dev).to(dt)
        dy = torch.randn(256,192,F//2,C,device=dev).to(dt)
        g,b = torch.ones(C,device=dev), torch.zeros(C,device=dev)
        st = ops.bn_train_stats(x, g, b, torch.zeros(C,device=dev), torch.ones(C,device=dev))
        dg, db = torch.zeros(C,device=dev), torch.zeros(C,device=dev)
        dx = torch.empty_like(x)
        y = torch.empty(256,192,F//2,C,device=dev,dtype=dt)
        wide = torch.empty(256,192,2,640,device=dev,dtype=dt)
        dwide = torch.randn(256,192,2,640,device=dev).to(dt)
        tap = ops.Tap(wide, tap_pool, coff, want_argmax=True)
        tap.grad = dwide
        f_bn = timed(lambda: ops.bn_act_pool_fwd(x, st, pool=2, out=y))
        f_tap = timed(lambda: ops.maxpool_fwd(x, tap_pool, out=wide, coff=coff, want_argmax=True))
        f_fused = timed(lambda: ops.bn_act_pool_fwd(x, st, pool=2, out=y, tap=tap))
        b_bn = timed(lambda: ops.bn_act_pool_bwd(x, dy, st, dg, db, pool=2, dx=dx))
        b_tap = timed(lambda: ops.maxpool_bwd_add(x, dwide, dx, tap_pool, coff=coff, argmax=tap.argmax))
        b_fused = timed(lambda: ops.bn_act_pool_bwd(x, dy, st, dg, db, pool=2, dx=dx, tap=tap))
        print(f"tap F={F} C={C} tap_pool={tap_pool} {'bf16' if a16 else 'fp32'}: "
              f"fwd bn {f_bn:.3f} + tap {f_tap:.3f} = {f_bn+f_tap:.3f} ms, fused {f_fused:.3f} ms   "
              f"bwd bn {b_bn:.3f} + tap {b_tap:.3f} = {b_bn+b_tap:.3f} ms, fused {b_fused:.3f} ms")
        del x, dy, dx, y, wide, dwide, tap
