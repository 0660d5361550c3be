"""Relation agreement on a real MI355X (csg_relation_agreement, csrc/metrics.hip) against its numpy restatement
(tests/agreement_cases.py, itself held to the reference's verdicts by tests/test_agreement_cases.py).  Flags and counts are
integers: every comparison is exact."""
import ctypes

import numpy as np
import pytest
import torch

import agreement_cases as ac
from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return torch.device("cuda:0")


def _device(case, cuda):
    boxes, centers, triplets, ttype, table = ac.make_case(case)
    dev = [None if a is None else torch.from_numpy(a).to(cuda) for a in (boxes, centers, triplets, ttype)]
    return (boxes, centers, triplets, ttype, table), dev


@pytest.mark.timeout(120)
@pytest.mark.parametrize("case", ac.CASES, ids=ac.case_id)
def test_every_case_equals_the_restatement(cuda, case):
    from canonicalsg2im_amd import _lib, ops
    assert hasattr(_lib.lib, "csg_relation_agreement")                   # the entry is found by its symbol
    host, (boxes, centers, triplets, ttype) = _device(case, cuda)
    table = host[4]
    vocab = ac.vocab_of(table)
    want_tested, want_agrees, want_per, want_totals = ac.restate(*host)
    totals = torch.zeros((4, len(table), 2), device=cuda, dtype=torch.int64)
    first = ops.relation_agreement(boxes, triplets, ttype, vocab, totals, centers=centers)
    once = totals.clone()
    second = ops.relation_agreement(boxes, triplets, ttype, vocab, totals, centers=centers,
                                    triplets_host=host[2], triplet_type_host=host[3])      # checked on the host too: all valid
    torch.cuda.synchronize()
    tested, agrees, per = (t.cpu().numpy() for t in first)
    print("%s: %d of %d rows tested, %d agree" % (ac.case_id(case), int(tested.sum()), tested.size, int(agrees.sum())))
    assert tested.dtype == np.uint8 and agrees.dtype == np.uint8 and per.dtype == np.int64
    assert np.array_equal(tested, want_tested) and np.array_equal(agrees, want_agrees) and np.array_equal(per, want_per)
    assert np.array_equal(once.cpu().numpy(), want_totals)
    assert np.array_equal(totals.cpu().numpy(), 2 * want_totals)                          # the call ADDS to the buffer
    for a, b in zip(first, second):                                                       # the same bits on every run
        assert torch.equal(a, b)


@pytest.mark.timeout(120)
def test_ground_truth_layouts_obey_their_own_original_triplets(cuda):
    """The invariant: with a batch's own ground-truth boxes and centres every tested triplet of type 0 agrees (the
    reference's batches, tests/golden/clevr_syn.npz part b)."""
    from canonicalsg2im_amd import ops
    meta, z = load_golden("clevr_syn")
    table = meta["pred_name_to_idx"]
    vocab = ac.vocab_of(table)
    totals = torch.zeros((4, 8, 2), device=cuda, dtype=torch.int64)
    want_totals = np.zeros((4, 8, 2), np.int64)
    for run in meta["runs"]:
        if run.get("getitem"):
            continue
        for lt in (0, 1):
            pre = "%s_lt%d_" % (run["key"], lt)
            boxes, centers = z[pre + "boxes"], z[pre + "centers"]
            triplets, ttype = z[pre + "triplets"].to(torch.int64), z[pre + "triplet_type"].to(torch.int64)
            tested, agrees, per = ops.relation_agreement(boxes.to(cuda), triplets.to(cuda), ttype.to(cuda), vocab, totals,
                                                         centers=centers.to(cuda))
            want = ac.restate(boxes.numpy(), centers.numpy(), triplets.numpy(), ttype.numpy(), table)
            want_totals += want[3]
            per = per.cpu().numpy()
            assert np.array_equal(tested.cpu().numpy(), want[0]) and np.array_equal(agrees.cpu().numpy(), want[1])
            assert np.array_equal(per, want[2])
            assert (per[:, 0, 0] == per[:, 0, 1]).all() and per[:, 0, 1].min() > 0
    assert np.array_equal(totals.cpu().numpy(), want_totals) and int(want_totals[0, :, 1].sum()) > 500
    assert (want_totals[0, :, 0] == want_totals[0, :, 1]).all() and (want_totals[:, :2] == 0).all()


@pytest.mark.timeout(120)
def test_rows_the_device_cannot_dereference_are_not_tested(cuda):
    """Without host copies a row that names an object outside [0, O) or a type outside [0, 4) is known on the device
    alone: it is never dereferenced and written as not tested; with the copies the call is refused before any launch."""
    from canonicalsg2im_amd import ops
    table, vocab = ac.PACKED, ac.vocab_of(ac.PACKED)
    boxes = torch.tensor([[[0.0, 0.0, 0.5, 0.5], [0.5, 0.5, 0.25, 0.25]]], device=cuda)
    above = table["__above__"]
    rows = [(0, above, 1), (2, above, 1), (0, above, -1), (1 << 40, above, 0), (0, above, 1), (0, table["__in_image__"], 7)]
    types = [0, 0, 0, 0, 4, 0]
    triplets, ttype = torch.tensor([rows], device=cuda), torch.tensor([types], device=cuda)
    totals = torch.zeros((4, 8, 2), device=cuda, dtype=torch.int64)
    tested, agrees, per = ops.relation_agreement(boxes, triplets, ttype, vocab, totals)
    torch.cuda.synchronize()
    assert tested.cpu().tolist() == [[1, 0, 0, 0, 0, 0]] and agrees.cpu().tolist() == [[1, 0, 0, 0, 0, 0]]
    assert per.cpu()[0, 0].tolist() == [1, 1] and int(totals.sum()) == 2 and totals[0, above].cpu().tolist() == [1, 1]
    for k, what in ((1, "names an object outside"), (2, "names an object outside"), (4, "type 4 outside")):
        keep = [0, k, 5]
        with pytest.raises(RuntimeError, match="csg_relation_agreement: triplet 1 of sample 0.*" + what):
            ops.relation_agreement(boxes, triplets[:, keep].contiguous(), ttype[:, keep].contiguous(), vocab, totals,
                                   triplets_host=triplets[:, keep].cpu(), triplet_type_host=ttype[:, keep].cpu())
    torch.cuda.synchronize()
    assert int(totals.sum()) == 2                                          # refused before the first launch


@pytest.mark.timeout(120)
def test_the_entry_refuses_before_any_launch(cuda):
    from canonicalsg2im_amd import _lib, ops
    call = _lib.lib.csg_relation_agreement
    buf = torch.zeros(4096, dtype=torch.int64, device=cuda)
    a = _lib.ptr(buf)
    ids = (ctypes.c_int32 * 8)(*range(8))
    ws = _lib.lib.csg_relation_agreement_workspace
    assert ws(1) == 24 * 2 * 8 and ws(3) == 3 * ws(1) and ws(0) == 0 and ws(65536) == 0

    def run(B=1, O=2, T=3, P=8, ids=ids, nbytes=4096 * 8, ptrs=None, host=(None, None)):
        p = [a] * 9 if ptrs is None else ptrs                 # boxes centers triplets type | tested agrees per totals ws
        return call(p[0], p[1], p[2], p[3], host[0], host[1], B, O, T, P, ids, p[4], p[5], p[6], p[7], p[8], nbytes, None)

    for kw in ({"B": 0}, {"B": 65536}, {"O": 0}, {"O": (1 << 20) + 1}, {"T": 0}, {"T": (1 << 20) + 1}, {"P": 0}, {"P": 4097}):
        assert run(**kw) == -1 and "csg_relation_agreement: bad shape" in _lib.last_error(), kw
    for k in (0, 2, 3, 4, 5, 6, 7, 8):                        # every operand but centers, which may be NULL
        assert run(ptrs=[None if i == k else a for i in range(9)]) == -1 and "null operand" in _lib.last_error()
    assert call(a, a, a, a, None, None, 1, 2, 3, 8, None, a, a, a, a, a, 4096 * 8, None) == -1 and "null operand" in _lib.last_error()
    odd = ctypes.c_void_p(buf.data_ptr() + 8)
    assert run(ptrs=[odd] + [a] * 8) == -1 and "16-byte aligned" in _lib.last_error()
    assert run(ptrs=[a, ctypes.c_void_p(buf.data_ptr() + 4)] + [a] * 7) == -1 and "8-byte aligned" in _lib.last_error()
    assert run(nbytes=ws(1) - 8) == -4 and "workspace" in _lib.last_error()
    assert run(P=7) == -1 and "outside [0, P = 7)" in _lib.last_error()
    assert run(ids=(ctypes.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, 6)) == -1 and "must be distinct" in _lib.last_error()
    assert run(ids=(ctypes.c_int32 * 8)(0, 1, 2, 3, 4, 5, 6, -1)) == -1 and "outside [0, P" in _lib.last_error()
    some = torch.zeros(9, dtype=torch.int64)
    assert run(host=(ctypes.c_void_p(some.data_ptr()), None)) == -1 and "come together" in _lib.last_error()
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0                                # nothing was launched: the buffer every output aliased is untouched
    # the Python face
    vocab = ac.vocab_of(ac.PACKED)
    good = dict(boxes=torch.zeros(1, 2, 4, device=cuda), triplets=torch.zeros(1, 3, 3, dtype=torch.int64, device=cuda),
                triplet_type=torch.zeros(1, 3, dtype=torch.int64, device=cuda), vocab=vocab,
                totals=torch.zeros(4, 8, 2, dtype=torch.int64, device=cuda))
    for change, what in (({"totals": torch.zeros(4, 8, 2, device=cuda)}, "totals must be a dense int64"),
                         ({"totals": torch.zeros(4, 9, 2, dtype=torch.int64, device=cuda)}, "totals must be a dense int64"),
                         ({"triplets": torch.zeros(1, 3, 3, dtype=torch.int32, device=cuda)}, "triplets must be"),
                         ({"boxes": torch.zeros(2, 2, 4, device=cuda)}, "boxes must be"),
                         ({"triplet_type": torch.zeros(1, 4, dtype=torch.int64, device=cuda)}, "triplet_type must be"),
                         ({"centers": torch.zeros(1, 3, 2, device=cuda)}, "centers must be"),
                         ({"boxes": torch.zeros(1, 2, 4)}, "no CPU path")):
        with pytest.raises(RuntimeError, match=what):
            ops.relation_agreement(**dict(good, **change))


@pytest.mark.timeout(120)
def test_stream_ordered_no_read_back_and_capturable(cuda):
    from canonicalsg2im_amd import ops
    case = (3, 257, 31, True, 1)
    host, (boxes, centers, triplets, ttype) = _device(case, cuda)
    vocab = ac.vocab_of(host[4])
    want = ac.restate(*host)
    totals = torch.zeros((4, len(host[4]), 2), device=cuda, dtype=torch.int64)
    ops.relation_agreement(boxes, triplets, ttype, vocab, totals, centers=centers)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                   # a synchronising call raises (where this torch build checks)
    try:
        ops.relation_agreement(boxes, triplets, ttype, vocab, totals, centers=centers)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert np.array_equal(totals.cpu().numpy(), 2 * want[3])
    totals.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ops.relation_agreement(boxes, triplets, ttype, vocab, totals, centers=centers)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(totals.cpu().numpy(), 3 * want[3])
    assert np.array_equal(outs[0].cpu().numpy(), want[0]) and np.array_equal(outs[1].cpu().numpy(), want[1])
    assert np.array_equal(outs[2].cpu().numpy(), want[2])
