"""Generate tests/golden/input_grad_golden.npz: the reference model's gradient of the training loss with respect to
its INPUT, in float64.

Run ONLY where the reference checkout is present (see make_golden.py):  python tests/golden/make_input_grad_golden.py
The reference's own ``model.JDCNet`` is loaded with ``seeded_state(11)`` and run on ``golden_input(3, T=T)`` /
``golden_targets(3, T=T)`` (B = 2) under torch autograd; the loss is ``oracle.model_ref.jdc_loss``.

  entry                      head                      mode                                   T
  bilstm_T32_eval_dx         BiLSTM (hidden 384)       eval                                   32
  bilstm_T32_train_dx        BiLSTM (hidden 384)       train, every dropout rate 0            32
  bilstm_T192_eval_dx        BiLSTM (hidden 384)       eval                                   192
  tf_T32_eval_dx             Transformer (TF_CFG)      eval                                   32
  tf_T32_train_dx            Transformer (TF_CFG)      train, every dropout rate 0            32

Next to each (head, T): ``<head>_T<T>_eval_grad_norms``, the float64 norms of the eval-mode parameter gradients (the
gradients ``nn.BatchNorm2d.eval()`` gives under autograd), in the order of ``<head>_grad_names``.
"""
import sys

import numpy as np
import torch

from make_golden import HERE, REF, SEQ_CFG, TF_CFG, disable_dropout, golden_input, golden_targets, ref_module

from oracle import model_ref  # noqa: E402  (make_golden put the repository root on sys.path)

SEED = 3
CASES = (("bilstm", 32, ("eval", "train")), ("bilstm", 192, ("eval",)), ("tf", 32, ("eval", "train")))


def head_config(head):
    """(seeded state, sequence_model_config) of a golden head."""
    if head == "tf":
        return model_ref.seeded_state(11, num_class=1, model_type="transformer"), dict(TF_CFG)
    return model_ref.seeded_state(11, num_class=1, hidden_size=384), dict(SEQ_CFG, hidden_size=384)


def reference_input_grad(ref_model_mod, head, T, mode):
    state, cfg = head_config(head)
    net = ref_model_mod.JDCNet(num_class=1, sequence_model_config=dict(cfg))
    net.load_state_dict(state, strict=True)
    disable_dropout(net)
    net = net.double()
    net.train(mode == "train")
    x = golden_input(SEED, T=T).double().requires_grad_(True)
    f0, sil = (t.double() for t in golden_targets(SEED, T=T))
    cls, det = net(x)                       # (grad mode on: the encoder takes its ordinary path, see make_golden.py)
    loss, _, _ = model_ref.jdc_loss(cls, det, f0, sil, 0.1)
    loss.backward()
    names = [n for n, _ in net.named_parameters()]
    norms = [p.grad.double().norm().item() for _, p in net.named_parameters()]
    return x.grad.numpy(), names, np.array(norms, dtype=np.float64)


if __name__ == "__main__":
    torch.set_num_threads(8)
    sys.path.insert(0, str(REF))
    ref_model = ref_module("ref_model", "model.py")
    out = {}
    for head, T, modes in CASES:
        for mode in modes:
            dx, names, norms = reference_input_grad(ref_model, head, T, mode)
            out[f"{head}_T{T}_{mode}_dx"] = dx
            if mode == "eval":
                out[f"{head}_T{T}_eval_grad_norms"] = norms
                out[f"{head}_grad_names"] = np.array(names)
            print(head, T, mode, dx.shape, float(np.abs(dx).max()), flush=True)
    np.savez_compressed(HERE / "input_grad_golden.npz", **out)
    print("input_grad_golden.npz", len(out), "arrays")
