"""The scene-graph encoder path matrix: one row per code path (and per kernel corner) of csrc/graph.hip that the public
entry points can reach (`ops.embed`, `ops.real_object_mask`, `ops.graph_csr`, `ops.gather_concat`, `ops.segment_avg` and
`GraphTripleConv` itself), with `graph_ref64`, a plain float64 CPU restatement of the family's contract (reference
sg2im/graph.py:60-106, sg2im/attribute_embed.py:38-45, sg2im/utils.py:56-63).  Used by tests/test_gpu_graph_paths.py (each
row through the entry point it names on the device) and tests/test_graph_cases.py (on the CPU: the reference against the
golden file the reference's own layer wrote, the host CSR loop against a second construction, the table's coverage of
every value the restated dispatch rules can return, the rows' own conditions).

A row (dict, built by `row`) holds
  name, family    — the id; "csr" | "seg" | "embed" | "mask" | "layer"
  csr rows        — B, O, T; bad: about 5 % of the subject / object ids are -1 or O (both builders drop such entries)
  seg rows        — B, O, T, H (hidden width: pooled is (B, O, H), h is (B, T, 2H + Dp)), Dp (predicate width, in and out), Din
                    (object width of gather_concat); graph: the builder (GRAPHS below); zero_conf: an object whose every
                    triplet has type 2 / 3 (confidence exactly 0); isolated: objects no triplet names; degrees: the "degrees"
                    builder's incident-edge count per object; relu: segment_avg(h_is_relu=...); new_p: whether new_p gets a
                    cotangent; need: which of ("obj", "pred", "h", "conf") require grad; seg_only: no gather_concat (Dp = 0)
  embed rows      — tables: ((num_emb, dim), ...); lead: the index tensor's leading shape (rows = prod(lead)); need: per table;
                    oob: two indices are out of range (-1 and num_emb)
  mask rows       — shape (B, O, A), image_id
  layer row       — the package's GraphTripleConv(Din, Din, Dp, Dp, H) on a `padded` + `zero_conf` graph
  kernels         — what the dispatch rules below give for the row, COMPUTED by `_kernels` from the row's own data
  expect          — star / padded rows: the segment count of the longest CSR row (a sparse-mode row: its edge count), typed in
                    (tests/test_graph_cases.py holds the computed one to it)
  refuse          — the call must raise a RuntimeError matching this pattern before any launch
  seed            — added to the data generator's seed (crc32 of the name): the layer row moves it until no ReLU
                    pre-activation lies near zero (tests/test_graph_cases.py)

No row excludes anything from its comparison.  `h` is data (a post-ReLU tensor with about half its entries exactly 0), so
the ReLU gate of `h_is_relu` has no kink ambiguity: the expected dh is the plain gradient times (h > 0)."""
import zlib

import torch
import torch.nn.functional as F

GRAPHS = ("random", "closure", "star", "padded", "degrees")
P = 8                          # predicate vocabulary of the rows (id 0: __padding__)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------- the dispatch rules
EMB_TILE_FLOATS, CSR_CHUNK, CSR_MAXJ, CSR_NCH, ROWSUM_SEG_EDGES = 8192, 2048, 4, 64, 128   # csrc/graph.hip:31,81,82,163,260


def emb_chunk_rows(dim):
    """Rows per block of k_embed_bwd (csrc/graph.hip:32-35)."""
    r = EMB_TILE_FLOATS // dim
    return 1024 if r > 1024 else (32 if r < 32 else r)


def emb_rule(rows, num_emb, dim):
    """csg_embed_bwd (csrc/graph.hip:612-634): chunk rows, chunk count (1: straight onto dtable, more: partials + the sum
    kernel), grid.y = 256-entry slabs of the table; dim > 256 is refused."""
    if dim > 256:
        return dict(refuse=True)                                                        # :612
    chunk = emb_chunk_rows(dim)                                                         # :617
    return dict(refuse=False, chunk=chunk, chunks=cdiv(rows, chunk), grid_y=cdiv(num_emb * dim, 256))   # :618-620


def csr_sorted_lds(T, O):
    """Dynamic LDS of k_csr_build_sorted (csrc/graph.hip:221-223)."""
    return 2 * O * CSR_NCH * 2 + (2 * O + O + 1) * 4 + 2 * T


def csr_builder(O, T):
    """csg_graph_csr_lds, which csg_graph_csr_build asks (csrc/graph.hip:648-652, :658-663): "refuse" | "sorted" (counting
    sort) | "plain"."""
    if O > 256 * CSR_MAXJ:                                                              # :649, :658
        return "refuse"
    if O <= 254 and 512 <= T <= 65535 and csr_sorted_lds(T, O) <= 150 * 1024:           # :651
        return "sorted"
    return "plain"


def rowsum_lpe(D):
    """Lanes per edge of k_csr_rowsum / k_rowsum_finish (csrc/graph.hip:457-461)."""
    l = 1
    while l * 4 < D and l < 256:
        l <<= 1
    return l


def rowsum_passes(D):
    """d0 passes of a group of LPE lanes over D columns (csrc/graph.hip:339, :419)."""
    return cdiv(D, rowsum_lpe(D) * 4)


def rowsum_nseg(O, T):
    """Segments per image in edge-balanced mode; 0 = sparse, one workgroup per row (csrc/graph.hip:464-468)."""
    deg = cdiv(2 * T, O) if O > 0 else 0
    if deg <= 48 or O > 1024:
        return 0
    return cdiv(2 * T, ROWSUM_SEG_EDGES) + O


def row_segments(n_edges):
    """Segments of one CSR row in edge-balanced mode: an empty row keeps one (csrc/graph.hip:294)."""
    return max(1, cdiv(n_edges, ROWSUM_SEG_EDGES))


def finish_groups(lpe):
    """Segment groups of k_rowsum_finish's 1024 threads (csrc/graph.hip:414)."""
    return 1024 // lpe


def finish_rule(dense, max_s, D):
    """"none": sparse mode, no finish launch (:712, :749); "idle": every row has one segment (:413); "single": every group
    adds at most one segment; "pairs": a group adds two or more, the two-accumulator loop runs (:424)."""
    if not dense:
        return "none"
    if max_s <= 1:
        return "idle"
    return "pairs" if max_s > finish_groups(rowsum_lpe(D)) else "single"


def row_lengths(tr, O):
    """(B, O): incident entries per object, out-of-range ids dropped."""
    B = tr.shape[0]
    out = torch.zeros(B, O, dtype=torch.int64)
    for b in range(B):
        ids = torch.cat([tr[b, :, 0], tr[b, :, 2]])
        ids = ids[(ids >= 0) & (ids < O)]
        out[b] = torch.bincount(ids, minlength=O)[:O]
    return out


def max_segments(c, d):
    return int(max(row_segments(int(n)) for n in row_lengths(d["tr"], c["O"]).flatten())) if c["O"] else 0


def _kernels(c, d):
    f = c["family"]
    if f == "mask":
        return "obj_mask"
    if f == "embed":
        rows = 1
        for n in c["lead"]:
            rows *= n
        out = []
        for (n, dim), need in zip(c["tables"], c["need"]):
            r = emb_rule(rows, n, dim)
            out.append("fwd" if not need else "refuse" if r["refuse"] else "chunk=%d chunks=%d gridy=%d" % (
                r["chunk"], r["chunks"], r["grid_y"]))
        return " | ".join(out)
    O, T = c["O"], c["T"]
    b = csr_builder(O, T)
    if f == "csr":
        return "csr=%s" % b + ("" if b != "plain" else " slots=%d stage=%d" % (cdiv(O, 256), cdiv(T, CSR_CHUNK)))
    dense = rowsum_nseg(O, T) > 0
    ms = max_segments(c, d) if dense else 1
    longest = int(row_lengths(d["tr"], O).max()) if O else 0
    s = "csr=%s rowsum=%s %s pooled:LPE=%dx%d finish=%s" % (
        b, "dense" if dense else "sparse", "maxS=%d" % ms if dense else "maxrow=%d" % longest, rowsum_lpe(c["H"]),
        rowsum_passes(c["H"]), finish_rule(dense, ms, c["H"]))
    if not c["seg_only"]:
        s += " dobj:LPE=%dx%d finish=%s" % (rowsum_lpe(c["Din"]), rowsum_passes(c["Din"]), finish_rule(dense, ms, c["Din"]))
    return s


# ------------------------------------------------------------------------------------------------- rows (the table: below)
def row(name, family, B=2, O=8, T=0, H=32, Dp=8, Din=16, graph="random", zero_conf=None, isolated=(), degrees=None, relu=True,
        new_p=True, need=("obj", "pred", "h", "conf"), seg_only=False, bad=False, tables=(), lead=(), oob=False, shape=None,
        image_id=0, expect=None, refuse=None, seed=0):
    assert family in ("csr", "seg", "embed", "mask", "layer") and graph in GRAPHS
    if graph == "closure":
        T = O * (O - 1)
    if family == "embed" and need == ("obj", "pred", "h", "conf"):
        need = (True,) * len(tables)
    c = dict(name=name, family=family, B=B, O=O, T=T, H=H, Dp=Dp, Din=Din, graph=graph, zero_conf=zero_conf,
             isolated=tuple(isolated), degrees=degrees, relu=relu, new_p=new_p, need=tuple(need), seg_only=seg_only, bad=bad,
             tables=tuple(tables), lead=tuple(lead), oob=oob, shape=shape, image_id=image_id, expect=expect, refuse=refuse,
             seed=seed)
    if family in ("seg", "layer"):
        assert H % 4 == 0 and Dp % 4 == 0 and Din % 4 == 0 and (Dp > 0 or seg_only)
        assert degrees is None or (len(degrees) == O and sum(degrees) == 2 * T)
    c["kernels"] = _kernels(c, dict(tr=_triplets(c, _gen(c))[0]) if family in ("seg", "layer") else None)   # (make_data's triplets)
    return c


def _both(name, **kw):
    """The row with h_is_relu = True (the model's call) and = False."""
    return [row(name + "_relu", "seg", relu=True, **kw), row(name + "_plain", "seg", relu=False, **kw)]


def case_ids(cases=None):
    return [c["name"] for c in (CASES if cases is None else cases)]          # (CASES: the end of this file)


# ------------------------------------------------------------------------------------------------- data
def _f32(t):
    """Values every precision can hold: the inputs of a row are float32 numbers."""
    return t.to(torch.float32).to(torch.float64)


def _gen(c):
    return torch.Generator().manual_seed((zlib.crc32(c["name"].encode()) + c["seed"]) & 0x7FFFFFFF)


def _triplets(c, g):
    """(tr (B, T, 3) int64 [s, p, o], valid (B, T) bool): p in [1, P) for real triplets, (0, 0, 0) for padding."""
    B, O, T = c["B"], c["O"], c["T"]
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g)
    valid = torch.ones(B, T, dtype=torch.bool)
    p = ri(1, P, B, T)
    if c["graph"] == "closure":
        pairs = torch.tensor([(s, o) for s in range(O) for o in range(O) if s != o], dtype=torch.int64).reshape(-1, 2)
        s, o = pairs[:, 0].expand(B, T).clone(), pairs[:, 1].expand(B, T).clone()
    elif c["graph"] == "star":                     # object 0 is the subject of every triplet and the object of all but every
        t = torch.arange(T)                        # 97th, which names one of the others: row 0 holds nearly all 2T entries
        s = torch.zeros(B, T, dtype=torch.int64)
        o = torch.where(t % 97 == 5, 1 + (t // 97) % (O - 1), torch.zeros_like(t)).expand(B, T).clone()
    elif c["graph"] == "degrees":                  # object i appears c["degrees"][i] times among the 2T endpoints
        ends = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(c["degrees"])])
        s, o = torch.empty(B, T, dtype=torch.int64), torch.empty(B, T, dtype=torch.int64)
        for b in range(B):
            e = ends[torch.randperm(2 * T, generator=g)]
            s[b], o[b] = e[:T], e[T:]
    else:
        pool = torch.tensor([i for i in range(O) if i not in c["isolated"]], dtype=torch.int64)
        s, o = pool[ri(0, len(pool), B, T)], pool[ri(0, len(pool), B, T)]
    if c["graph"] == "padded":                     # image b keeps a shrinking prefix; the last image keeps none
        for b in range(B):
            keep = T * (B - 1 - b) // (B - 1)
            s[b, keep:], o[b, keep:], p[b, keep:], valid[b, keep:] = 0, 0, 0, False
    return torch.stack([s, p, o], -1).contiguous(), valid


def make_data(c):
    """The row's inputs and cotangents: float64 CPU tensors holding float32 values, int64 indices."""
    g = _gen(c)
    rn = lambda *s: _f32(torch.randn(*s, generator=g, dtype=torch.float64))
    f = c["family"]
    if f == "mask":
        objs = torch.randint(0, 5, c["shape"], generator=g)
        return dict(objs=objs)
    if f == "embed":
        tabs = [rn(n, dim) for (n, dim) in c["tables"]]
        idx = torch.stack([torch.randint(0, n, c["lead"], generator=g) for (n, _) in c["tables"]], -1)
        if c["oob"]:
            flat = idx.view(-1, idx.shape[-1])
            flat[3, 0], flat[flat.shape[0] - 2, 0] = -1, c["tables"][0][0]
        return dict(tables=tabs, idx=idx, dout=rn(*c["lead"], sum(dim for (_, dim) in c["tables"])))
    B, O, T = c["B"], c["O"], c["T"]
    if f == "csr":
        tr = torch.stack([torch.randint(0, O, (B, T), generator=g), torch.randint(0, P, (B, T), generator=g),
                          torch.randint(0, O, (B, T), generator=g)], -1)
        if c["bad"]:
            for col in (0, 2):
                r = torch.rand(B, T, generator=g)
                tr[..., col] = torch.where(r < 0.025, torch.full_like(tr[..., col], -1),
                                           torch.where(r < 0.05, torch.full_like(tr[..., col], O), tr[..., col]))
        return dict(tr=tr.contiguous())
    H, Dp, Din = c["H"], c["Dp"], c["Din"]
    tr, valid = _triplets(c, g)
    tt = torch.randint(0, 4, (B, T), generator=g)
    tt[~valid] = 0                                 # the collate's padding: type 0, so conf = 1 on an invalid triplet
    if c["zero_conf"] is not None:
        z = (tr[..., 0] == c["zero_conf"]) | (tr[..., 2] == c["zero_conf"])
        tt = torch.where(z & valid, 2 + (torch.arange(T) % 2).expand(B, T), tt)
    w_trans = rn(P)
    conf32 = (tt == 0).float() + (tt == 1).float() * torch.sigmoid(w_trans.float())[tr[..., 1]]   # graph.py:70-74, in float32
    d = dict(tr=tr, valid=valid, tt=tt, w_trans=w_trans, conf=conf32.double(), obj=rn(B, O, Din), pred=rn(B, T, Dp),
             h=_f32(torch.relu(torch.randn(B, T, 2 * H + Dp, generator=g, dtype=torch.float64))),
             dcat=rn(B, T, 2 * Din + Dp), dpooled=rn(B, O, H), dnew_p=rn(B, T, Dp))
    if f == "layer":
        d.update(dnew_obj=rn(B, O, Din), sd=layer_state(c))
    return d


def layer_state(c):
    """The package's own layer, seeded: {parameter name: float64 CPU tensor holding float32 values}."""
    from canonicalsg2im_amd.sg2im.graph import GraphTripleConv, get_predicates_weights
    torch.manual_seed((zlib.crc32(c["name"].encode()) + c["seed"]) & 0x7FFFFFFF)
    m = GraphTripleConv(c["Din"], c["Din"], c["Dp"], c["Dp"], c["H"], 1,
                        predicates_transitive_weights=get_predicates_weights(P, "uniform"))
    sd = {k: _f32(v.detach()) for k, v in m.state_dict().items()}
    for k in list(sd):                             # kaiming weights; biases that matter
        if k.endswith(".bias"):
            sd[k] = _f32(0.1 * torch.randn(sd[k].shape, dtype=torch.float64))
    return sd


# ------------------------------------------------------------------------------------------------- the host CSR, twice
def csr_host(tr, O):
    """(row_ptr (B, O + 1), col (B, max(2T, 1))) int32: per object its subject entries 2t in t order, then its object
    entries 2t + 1 in t order (the order of graph.py:98-99); an id outside [0, O) has no row and is dropped."""
    B, T, _ = tr.shape
    rp = torch.zeros(B, O + 1, dtype=torch.int32)
    col = torch.zeros(B, max(2 * T, 1), dtype=torch.int32)
    trl = tr.tolist()
    for b in range(B):
        rows = [[] for _ in range(O)]
        for role in (0, 1):
            for t in range(T):
                i = trl[b][t][2 * role]
                if 0 <= i < O:
                    rows[i].append(2 * t + role)
        flat = [e for r in rows for e in r]
        pos = 0
        for i in range(O):
            rp[b, i] = pos
            pos += len(rows[i])
        rp[b, O] = pos
        col[b, :pos] = torch.tensor(flat, dtype=torch.int32)
    return rp, col


def csr_argsort(tr, O):
    """The same arrays from a stable sort of the 2T (object, role, t) keys."""
    B, T, _ = tr.shape
    rp = torch.zeros(B, O + 1, dtype=torch.int32)
    col = torch.zeros(B, max(2 * T, 1), dtype=torch.int32)
    for b in range(B):
        ids = torch.cat([tr[b, :, 0], tr[b, :, 2]])                       # role-major: entry e = role * T + t
        code = torch.cat([2 * torch.arange(T), 2 * torch.arange(T) + 1])
        ok = (ids >= 0) & (ids < O)
        ids, code = ids[ok], code[ok]
        order = torch.argsort(ids, stable=True)
        n = int(ok.sum())
        col[b, :n] = code[order].to(torch.int32)
        rp[b, 1:] = torch.cumsum(torch.bincount(ids, minlength=O)[:O], 0).to(torch.int32)
    return rp, col


# ------------------------------------------------------------------------------------------------- graph_ref64
def gather_ref(obj, pred, tr):
    """graph.py:60-66: cat(obj[s], pred, obj[o])."""
    Din = obj.shape[-1]
    return torch.cat([torch.gather(obj, 1, tr[..., 0:1].expand(-1, -1, Din)), pred,
                      torch.gather(obj, 1, tr[..., 2:3].expand(-1, -1, Din))], -1)


def segavg_ref(h, conf, valid, tr, O, H, Dp):
    """graph.py:76-109: (pooled (B, O, H), new_p (B, T, Dp)) — the confidence-scaled messages of the valid triplets added per
    object with index_add, per image, then a true division where the summed confidence is > 0."""
    B = h.shape[0]
    new_t = h * conf.unsqueeze(-1)                                        # :77
    pooled = []
    for b in range(B):
        m = valid[b]
        s_i, o_i = tr[b, m, 0], tr[b, m, 2]
        acc = torch.zeros(O, H, dtype=h.dtype).index_add(0, s_i, new_t[b, m, :H]).index_add(0, o_i, new_t[b, m, H + Dp:])
        cnt = torch.zeros(O, dtype=h.dtype).index_add(0, s_i, conf[b, m]).index_add(0, o_i, conf[b, m])
        nz = cnt > 0                                                      # :105-106
        pooled.append(acc / torch.where(nz, cnt, torch.ones_like(cnt)).unsqueeze(-1))
    return torch.stack(pooled), new_t[..., H:H + Dp]


def confidence(tt, w_trans, p):
    """graph.py:70-74"""
    return (tt == 0).to(w_trans.dtype) + (tt == 1).to(w_trans.dtype) * torch.sigmoid(w_trans)[p]


def layer_ref(sd, obj, pred, tr, tt, valid, H, Dp, detail=None):
    """GraphTripleConv.forward (graph.py:44-113) from a state dict: (new_obj, new_p)."""
    cat = gather_ref(obj, pred, tr)
    pre1 = F.linear(cat, sd["net1.0.weight"], sd["net1.0.bias"])
    pre2 = F.linear(torch.relu(pre1), sd["net1.2.weight"], sd["net1.2.bias"])
    conf = confidence(tt, sd["predicates_transitive_weights"], tr[..., 1])
    pooled, new_p = segavg_ref(torch.relu(pre2), conf, valid, tr, obj.shape[1], H, Dp)
    pre3 = F.linear(pooled, sd["net2.0.weight"], sd["net2.0.bias"])
    pre4 = F.linear(torch.relu(pre3), sd["net2.2.weight"], sd["net2.2.bias"])
    if detail is not None:
        detail.update({"net1.0": pre1.detach(), "net1.2": pre2.detach(), "net2.0": pre3.detach(), "net2.2": pre4.detach()})
    return torch.relu(pre4), new_p


LAYER_PARAMS = ("net1.0.weight", "net1.0.bias", "net1.2.weight", "net1.2.bias", "net2.0.weight", "net2.0.bias",
                "net2.2.weight", "net2.2.bias")


def _leaf(t, dtype, grad=True):
    return t.detach().clone().to(dtype).requires_grad_(grad)


def graph_ref64(c, d, dtype=torch.float64):
    """{tensor name: tensor or None}: every output of the row and every gradient it asks for, by name — cat, pooled, new_p,
    dobj, dpred, dh, dconf (seg rows); out, dtable_k (embed rows); mask; row_ptr, col (csr rows); new_obj, new_p, dobj, dpred,
    dw_trans and d<parameter> (the layer row).  `dtype=torch.float32` is the float32 CPU yardstick of the bands."""
    f = c["family"]
    if f == "mask":
        v = d["objs"][..., 0]
        return dict(mask=((v != 0) & (v != c["image_id"])).to(torch.uint8))                  # utils.py:56-63
    if f == "csr":
        rp, col = csr_host(d["tr"], c["O"])
        return dict(row_ptr=rp, col=col)
    if f == "embed":
        tabs = [_leaf(t, dtype, need) for t, need in zip(d["tables"], c["need"])]
        outs = []
        for k, t in enumerate(tabs):                                                          # attribute_embed.py:40-45
            i = d["idx"][..., k]
            ok = (i >= 0) & (i < t.shape[0])
            e = F.embedding(i.clamp(0, t.shape[0] - 1), t)
            outs.append(torch.where(ok.unsqueeze(-1), e, torch.full_like(e, float("nan"))))   # a bad index: NaN, no gradient
        out = torch.cat(outs, -1)
        res = dict(out=out.detach())
        if out.requires_grad:
            out.backward(d["dout"].to(dtype))
        for k, t in enumerate(tabs):
            res["dtable_%d" % k] = t.grad if c["need"][k] else None
        return res
    B, O, T, H, Dp = c["B"], c["O"], c["T"], c["H"], c["Dp"]
    tr, valid = d["tr"], d["valid"]
    if f == "layer":
        sd = {k: _leaf(v, dtype) for k, v in d["sd"].items()}
        obj, pred = _leaf(d["obj"], dtype), _leaf(d["pred"], dtype)
        new_obj, new_p = layer_ref(sd, obj, pred, tr, d["tt"], valid, H, Dp)
        ((new_obj * d["dnew_obj"].to(dtype)).sum() + (new_p * d["dnew_p"].to(dtype)).sum()).backward()
        res = dict(new_obj=new_obj.detach(), new_p=new_p.detach(), dobj=obj.grad, dpred=pred.grad,
                   dw_trans=sd["predicates_transitive_weights"].grad)
        res.update({"d" + k: sd[k].grad for k in LAYER_PARAMS})
        return res
    need = c["need"]
    res = dict(cat=None, dobj=None, dpred=None)
    if not c["seg_only"]:
        obj, pred = _leaf(d["obj"], dtype, "obj" in need), _leaf(d["pred"], dtype, "pred" in need)
        cat = gather_ref(obj, pred, tr)
        if cat.requires_grad and cat.numel():
            (cat * d["dcat"].to(dtype)).sum().backward()
        res.update(cat=cat.detach(), dobj=_grad(obj, "obj" in need), dpred=_grad(pred, "pred" in need))
    h, conf = _leaf(d["h"], dtype, "h" in need), _leaf(d["conf"], dtype, "conf" in need)
    pooled, new_p = segavg_ref(h, conf, valid, tr, O, H, Dp)
    loss = (pooled * d["dpooled"].to(dtype)).sum()
    if c["new_p"]:
        loss = loss + (new_p * d["dnew_p"].to(dtype)).sum()
    if loss.requires_grad:
        loss.backward()
    dh = _grad(h, "h" in need)
    if dh is not None and c["relu"]:
        dh = dh * (h.detach() > 0).to(dtype)       # h_is_relu: the gradient of the ReLU's pre-activation
    res.update(pooled=pooled.detach(), new_p=new_p.detach(), dh=dh, dconf=_grad(conf, "conf" in need))
    return res


def _grad(leaf, asked):
    if not asked:
        return None
    return leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)


def relu_margin(c, d):
    """The layer row's condition: the smallest |pre-activation| of every ReLU of the layer as a fraction of that tensor's
    largest magnitude, {ReLU name: fraction}, from the float64 reference alone."""
    detail = {}
    layer_ref({k: v for k, v in d["sd"].items()}, d["obj"], d["pred"], d["tr"], d["tt"], d["valid"], c["H"], c["Dp"], detail)
    return {k: float(v.abs().min() / v.abs().max()) for k, v in detail.items()}


# ------------------------------------------------------------------------------------------------- the rows
CASES = [
    # ---- the CSR builders: bit-exact row_ptr and col[:, :row_ptr[O]] against the host loop
    row("csr_o5_t511", "csr", O=5, T=511),                       # T = 511 | 512: plain | counting sort
    row("csr_o5_t512", "csr", O=5, T=512),
    row("csr_o3_t65535", "csr", O=3, T=65535),                   # T = 65535 | 65536: the 16-bit chunk offsets' limit
    row("csr_o3_t65536", "csr", O=3, T=65536),
    row("csr_o254_t600", "csr", O=254, T=600),                   # O = 254 | 255: the byte-sized (s, o) staging (255 = none)
    row("csr_o255_t600", "csr", O=255, T=600),
    row("csr_o254_t45000", "csr", O=254, T=45000),               # 155 KB of LDS > 150 KB: the plain builder
    row("csr_o300_t2048", "csr", O=300, T=2048),                 # one staging chunk | two
    row("csr_o300_t2049", "csr", O=300, T=2049),
    row("csr_o1024_t300", "csr", O=1024, T=300),                 # the fourth object slot of a thread
    row("csr_o1_t513", "csr", O=1, T=513),
    row("csr_o4_t0", "csr", O=4, T=0),
    row("csr_bad_o40_t700", "csr", O=40, T=700, bad=True),       # counting sort: the int64 is range-checked
    row("csr_bad_o300_t700", "csr", O=300, T=700, bad=True),     # plain: the id is truncated to int and never matches
    row("refuse_csr_o1025", "csr", O=1025, T=300, refuse="1024 objects per image"),
    # ---- CSR row sums and the segment average, both directions
    *_both("seg_o8_t192", O=8, T=192),                           # deg = ceil(2T / O) = 48: sparse
    *_both("seg_o8_t193", O=8, T=193),                           # 49: edge-balanced
    *_both("seg_deg_128_129_0", O=6, T=300, graph="degrees", degrees=(128, 129, 0, 115, 114, 114)),   # 1, 2, 1 segments
    *_both("seg_star_o6_t4200_h128", O=6, T=4200, H=128, graph="star", expect=66),    # 66 segments, 32 finish groups
    *_both("seg_star_o6_t600_h516", O=6, T=600, H=516, graph="star", expect=10),      # 10 segments, 4 finish groups
    row("seg_padded_sparse", "seg", B=3, O=40, T=900, graph="padded", expect=1800),   # a 1 800-edge hub in ONE workgroup
    row("seg_padded_dense", "seg", B=3, O=6, T=600, graph="padded", expect=10),
    row("seg_closure_o9_h2048", "seg", O=9, H=2048, Dp=16, Din=12, graph="closure"),
    row("seg_h4", "seg", O=7, T=25, H=4, Dp=4, Din=4),                                # LPE = 1: 256 edge groups
    row("seg_h4_dense", "seg", O=3, T=200, H=4, Dp=4, Din=4, relu=False),             # ... and 256 finish groups
    row("seg_h12", "seg", O=7, T=25, H=12, Dp=4, Din=12),                             # LPE = 4, one dead lane
    row("seg_h12_dense", "seg", O=3, T=300, H=12, Dp=4, Din=12),
    row("seg_h1028", "seg", O=7, T=25, H=1028, Dp=4, Din=8),                          # second d0 pass, one live lane
    row("seg_h1028_dense", "seg", O=3, T=200, H=1028, Dp=4, Din=8),
    row("seg_h260", "seg", O=7, T=25, H=260, Dp=260, Din=8),                          # second lane pass of k_segment_avg_bwd
    row("seg_zero_conf_sparse", "seg", O=8, T=40, zero_conf=2),
    row("seg_zero_conf_dense", "seg", O=6, T=500, zero_conf=2),
    row("seg_isolated", "seg", O=10, T=30, isolated=(0, 3, 9)),
    row("seg_isolated_dense", "seg", O=5, T=250, isolated=(0, 3), relu=False),        # an empty row keeps one segment
    row("seg_new_p_unused", "seg", O=8, T=40, new_p=False),
    row("seg_need_obj_h", "seg", O=8, T=40, need=("obj", "h")),                       # dpred and dconf must be None
    row("seg_dp0", "seg", O=8, T=40, Dp=0, seg_only=True),
    row("seg_dp0_dense", "seg", O=4, T=300, Dp=0, seg_only=True, relu=False),
    row("seg_t0", "seg", O=5, T=0),
    # ---- embedding lookups
    row("emb_8x8_r1024", "embed", tables=((8, 8),), lead=(1024,)),                    # one chunk: straight onto dtable
    row("emb_8x8_r1025", "embed", tables=((8, 8),), lead=(1025,)),                    # two: partials + the sum kernel
    row("emb_179x128_r300", "embed", tables=((179, 128),), lead=(3, 100)),            # the VG vocabulary: grid.y = 90
    row("emb_4x256_r70", "embed", tables=((4, 256),), lead=(70,)),                    # 32-row chunks
    row("emb_8x32_r27000", "embed", tables=((8, 32),), lead=(3, 9000)),               # dense graphs' predicate rows
    row("emb_four_tables", "embed", tables=((4, 8), (9, 16), (3, 4), (300, 12)), lead=(3, 11)),
    row("emb_two_tables_one_grad", "embed", tables=((5, 8), (6, 8)), lead=(40,), need=(False, True)),
    row("emb_dim300_fwd", "embed", tables=((6, 300),), lead=(20,), need=(False,)),
    row("refuse_emb_dim300", "embed", tables=((6, 300),), lead=(20,), refuse="embedding_dim <= 256"),
    row("emb_out_of_range", "embed", tables=((7, 8),), lead=(50,), oob=True),
    # ---- the real-object mask
    row("mask_5x13x3", "mask", shape=(5, 13, 3), image_id=0),
    row("mask_1x1025x1", "mask", shape=(1, 1025, 1), image_id=2),
    # ---- the layer itself: grad_is_pre on net1's last Linear and gate_relu in the segment average must compose
    row("layer_padded_zero_conf", "layer", B=3, O=12, T=40, H=64, Dp=32, Din=32, graph="padded", zero_conf=3, seed=1),
]
