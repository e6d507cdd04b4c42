"""CPU-side checks of the classification entry points (include/vitmi.h: vitmi_softmax_xent,
vitmi_mix_batch): host validation rejects bad arguments with a message before any launch."""
from vitmi import _lib

OK_PTR = 4096          # never dereferenced: every call below fails validation first


def rejected(rc, *words):
    msg = _lib.lib().vitmi_last_error()
    assert rc == 1, (rc, msg)
    assert msg and any(w in msg for w in words), msg


def xent(B=8, C=10, logits=OK_PTR, ldl=None, la=OK_PTR, lb=None, lam=None, soft=None, lds=None, smoothing=0.0,
         topk=0, row=OK_PTR, loss=OK_PTR, dl=OK_PTR, lddl=None, metrics=None, ws=OK_PTR, ws_bytes=1 << 20):
    return _lib.lib().vitmi_softmax_xent(B, C, logits, C if ldl is None else ldl, la, lb, lam, soft,
                                         C if lds is None else lds, smoothing, topk, row, loss, dl,
                                         C if lddl is None else lddl, metrics, ws, ws_bytes, None)


def test_workspace_size_is_pure_host():
    lib = _lib.lib()
    assert lib.vitmi_softmax_xent_workspace_size(0) == 0
    assert lib.vitmi_softmax_xent_workspace_size(1) == 32
    assert lib.vitmi_softmax_xent_workspace_size(256) == 256 * 4 + 256
    assert lib.vitmi_softmax_xent_workspace_size(37) >= 37 * 5


def test_xent_rejects_bad_shapes():
    rejected(xent(B=0), b"B must")
    rejected(xent(C=0), b"C must")
    rejected(xent(C=65536), b"C must")
    rejected(xent(ldl=9), b"ldl")
    rejected(xent(lddl=9), b"lddl")
    rejected(xent(soft=OK_PTR, la=None, lds=9), b"lds")
    rejected(xent(logits=None), b"null logits")


def test_xent_rejects_bad_hyper_parameters():
    rejected(xent(smoothing=1.0), b"smoothing")
    rejected(xent(smoothing=-0.1), b"smoothing")
    rejected(xent(smoothing=float("nan")), b"smoothing")
    rejected(xent(topk=11), b"topk")
    rejected(xent(topk=-1), b"topk")
    rejected(xent(topk=0, metrics=OK_PTR), b"topk")


def test_xent_rejects_bad_pointer_combinations():
    rejected(xent(lam=OK_PTR), b"go together")                       # lam without label_b
    rejected(xent(lb=OK_PTR), b"go together")
    rejected(xent(la=None), b"label_a")                              # neither labels nor a dense target
    rejected(xent(soft=OK_PTR, lb=OK_PTR, lam=OK_PTR), b"dense")
    rejected(xent(soft=OK_PTR, la=None, metrics=OK_PTR, topk=1), b"label_a")   # metrics without label_a
    rejected(xent(metrics=OK_PTR + 8, topk=1), b"16-byte")           # metrics misaligned
    rejected(xent(row=None, loss=None, dl=None), b"every output")    # all outputs NULL
    rejected(xent(row=None, ws=None), b"workspace")                  # loss needs somewhere to fold from
    rejected(xent(metrics=OK_PTR, topk=1, ws_bytes=8), b"workspace")


def mix(B=2, C=3, H=8, W=8, img=OK_PTR, perm=OK_PTR, lam=OK_PTR, box=OK_PTR, out=1 << 20):
    return _lib.lib().vitmi_mix_batch(B, C, H, W, img, perm, lam, box, out, None)


def test_mix_rejects_bad_arguments():
    for name in ("B", "C", "H", "W"):
        rejected(mix(**{name: 0}), b"positive")
        rejected(mix(**{name: -3}), b"positive")
    for name in ("img", "perm", "lam", "box", "out"):
        rejected(mix(**{name: None}), b"null")
    rejected(mix(out=OK_PTR), b"alias")                              # out == img
    rejected(mix(out=OK_PTR + 2 * 3 * 8 * 8 * 4 - 4), b"alias")      # overlapping the last element
