"""The reference's occupancy octree (src/pointcloudmapping.cc:198-278) restated operation by operation, DESIGN.md §3 items 14-15:
pcl::transformPointCloud with a float 4x4, octomap::OcTree(res).updateNode(point, true) per point, and writeBinary (toMaxLikelihood,
prune, the header, the preorder two-bytes-per-inner-node data).

The tree is built the way octomap builds it: one descent per point into nested nodes, a recursive prune, a recursive preorder write -
deliberately not the sort the GPU uses.  levelwise() is a numpy form of the same tree for maps too large for the recursion; the CPU
test holds the two against each other.
"""
import numpy as np

F32 = np.float32
DEPTH = 16
CENTRE = 32768   # tree_max_val

# transform_trans, transform_rot_x, transform_rot_y (:198-223), and their product the reference hands to transformPointCloud (:247)
TRANS = np.array([[0, 1, 0, 0], [0, 0, -1, 0], [-1, 0, 0, 0], [0, 0, 0, 1]], F32)
ROT_X = np.array([[0, 1, 0, 0], [-1, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F32)
ROT_Y = np.array([[0, 0, -1, 0], [0, 1, 0, 0], [1, 0, 0, 0], [0, 0, 0, 1]], F32)
AXIS_SWAP = np.array([[0, 0, 1, 0], [-1, 0, 0, 0], [0, -1, 0, 0], [0, 0, 0, 1]], F32)
IDENTITY = np.eye(4, dtype=F32)

HEADER = ("# Octomap OcTree binary file\n# (feel free to add / change comments, but leave the first line as it is!)\n#\n"
          "id OcTree\nsize %d\nres %s\ndata\n")


def header(size, res):
    return (HEADER % (size, "%g" % res)).encode()


def transform(xyz, M):
    """pcl::transformPointCloud (PCL 1.8) of a cloud that is not dense: [n, 3] float32 -> (transformed [n, 3] float32, finite mask).
    A point with a non-finite coordinate is not transformed; the caller drops it."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    M = np.asarray(M, F32).reshape(4, 4)
    fin = np.isfinite(xyz).all(axis=1)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty_like(xyz)
    with np.errstate(all="ignore"):
        for r in range(3):   # every product and every sum rounded to float, left to right
            out[:, r] = ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]   # (float32 throughout)
    return out, fin


def keys(xyz, res):
    """coordToKeyChecked per point: [n, 3] float32 -> (int64 keys [n, 3], valid mask)."""
    res_factor = 1.0 / float(res)
    with np.errstate(all="ignore"):
        t = np.floor(res_factor * np.asarray(xyz, F32).astype(np.float64))
    ok = np.isfinite(t)
    k = np.where(ok, t, 0).astype(np.int64) + CENTRE
    ok &= (k >= 0) & (k <= 65535)
    return k, ok.all(axis=1)


def point_keys(xyz, M, res):
    """Points -> (the keys of the points that reach the tree, in input order; the number dropped)."""
    p, fin = transform(xyz, M)
    k, ok = keys(p, res)
    ok &= fin
    return k[ok], int((~ok).sum())


# ---- the tree, as octomap builds it

def build(key_rows):
    """updateNode(key, true) per point: a node is the dict of its children by index; a depth-16 node has none."""
    root = None
    for kx, ky, kz in key_rows:
        kx, ky, kz = int(kx), int(ky), int(kz)
        if root is None:
            root = {}
        node = root
        for d in range(DEPTH):
            b = DEPTH - 1 - d
            idx = ((kx >> b) & 1) | (((ky >> b) & 1) << 1) | (((kz >> b) & 1) << 2)
            node = node.setdefault(idx, {})
    return root


def prune(node, depth=0):
    """toMaxLikelihood (every leaf to the clamping maximum: all values equal) then prune(): a node of depth >= 1 whose eight children
    all exist and have no children becomes a leaf.  Bottom-up, which is what octomap's passes for depths 15 .. 1 amount to."""
    if node is None:
        return
    for c in node.values():
        prune(c, depth + 1)
    if depth >= 1 and len(node) == 8 and all(len(c) == 0 for c in node.values()):
        node.clear()


def size(node):
    return 0 if node is None else 1 + sum(size(c) for c in node.values())


def data_bytes(node):
    """writeBinaryNode: preorder over the nodes with children, two bytes each."""
    out = bytearray()

    def rec(n):
        bits = 0
        for i in range(8):
            if i in n:
                bits |= (3 if n[i] else 2) << (2 * i)
        out.append(bits & 255)
        out.append(bits >> 8)
        for i in range(8):
            if i in n and n[i]:
                rec(n[i])

    if node:
        rec(node)
    return bytes(out)


def leaves(node):
    """The leaves in preorder: rows (kx, ky, kz, depth), the key of the minimum corner."""
    out = []

    def rec(n, kx, ky, kz, depth):
        if not n:
            out.append((kx, ky, kz, depth))
            return
        b = DEPTH - 1 - depth
        for i in range(8):
            if i in n:
                rec(n[i], kx | ((i & 1) << b), ky | (((i >> 1) & 1) << b), kz | (((i >> 2) & 1) << b), depth + 1)

    if node:
        rec(node, 0, 0, 0, 0)
    return np.array(out, np.int64).reshape(-1, 4)


def octomap(xyz, M=AXIS_SWAP, res=0.1):
    """-> dict: data, leaves [n, 4], file (header + data) and every field of orbx_octree_info_t."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    k, dropped = point_keys(xyz, M, res)
    root = build(k)
    cells = len({tuple(r) for r in k.tolist()})
    prune(root)
    return _result(len(xyz), dropped, cells, size(root), data_bytes(root), leaves(root), res)


def _result(n_in, dropped, cells, tree_size, data, lv, res):
    return dict(points_in=n_in, points_dropped=dropped, cells=cells, leaves=len(lv), tree_size=tree_size, data_bytes=len(data),
                data=data, leaf_rows=lv, file=header(tree_size, res) + data)


def read_bt(buf):
    """The bytes of a .bt file -> (size, res, set of (kx, ky, kz, depth) leaves), as OcTree::readBinary walks them."""
    buf = bytes(buf)
    assert buf.startswith(b"# Octomap OcTree binary file\n")
    end = buf.index(b"\ndata\n") + 6
    fields = dict(l.split(" ", 1) for l in buf[:end].decode().splitlines() if l and not l.startswith("#") and " " in l)
    assert fields["id"] == "OcTree"
    n, res, data = int(fields["size"]), float(fields["res"]), buf[end:]
    out, pos = set(), 0
    if n == 0:
        assert not data
        return n, res, out
    stack = [(0, 0, 0, 0)]   # preorder: children pushed in reverse
    while stack:
        kx, ky, kz, depth = stack.pop()
        bits = data[pos] | (data[pos + 1] << 8)
        pos += 2
        b = DEPTH - 1 - depth
        inner = []
        for i in range(8):
            s = (bits >> (2 * i)) & 3
            child = (kx | ((i & 1) << b), ky | (((i >> 1) & 1) << b), kz | (((i >> 2) & 1) << b), depth + 1)
            assert s != 1, "a free leaf"
            if s == 2:
                out.add(child)
            elif s == 3:
                assert depth + 1 < DEPTH
                inner.append(child)
        stack.extend(reversed(inner))
    assert pos == len(data), "trailing bytes"
    return n, res, out


# ---- the same tree level by level in numpy (large maps)

def morton(k):
    """[n, 3] keys -> uint64 codes: the child index at depth d sits at bits 3(15-d) .. 3(15-d)+2, so ascending code is preorder."""
    k = np.asarray(k, np.uint64)
    c = np.zeros(len(k), np.uint64)
    for b in range(DEPTH):
        for a in range(3):
            c |= ((k[:, a] >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b + a)
    return c


def unmorton(c):
    c = np.asarray(c, np.uint64)
    k = np.zeros((len(c), 3), np.int64)
    for b in range(DEPTH):
        for a in range(3):
            k[:, a] |= (((c >> np.uint64(3 * b + a)) & np.uint64(1)) << np.uint64(b)).astype(np.int64)
    return k


def levelwise(xyz, M=AXIS_SWAP, res=0.1):
    """octomap() without the recursion: level 16 is the set of occupied cells; the parents of a level are the distinct code >> 3; a
    parent of depth >= 1 with eight children that are all leaves becomes a leaf of the level above and its children vanish."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    k, dropped = point_keys(xyz, M, res)
    code = np.unique(morton(k))            # depth-16 nodes
    cells = len(code)
    is_leaf = np.ones(len(code), bool)
    inner, leaf = [], []                   # (code aligned to depth 16, depth, two bytes) / (aligned code, depth)
    for d in range(DEPTH - 1, -1, -1):     # parents of depth d over children of depth d + 1
        if len(code) == 0:
            break
        pc, first = np.unique(code >> np.uint64(3), return_index=True)
        idx = (code & np.uint64(7)).astype(np.int64)
        status = np.where(is_leaf, 2, 3).astype(np.int64) << (2 * idx)
        bits = np.bitwise_or.reduceat(status, first)
        nchild = np.diff(np.append(first, len(code)))
        all_leaf = np.minimum.reduceat(is_leaf.astype(np.int64), first) == 1
        pruned = (nchild == 8) & all_leaf & (d >= 1)
        keep = ~np.repeat(pruned, nchild)   # children of a pruned parent vanish
        sh = np.uint64(3 * (DEPTH - 1 - d))
        for c in code[keep & is_leaf]:
            leaf.append((int(c << sh), d + 1))
        for c, b in zip(pc[~pruned], bits[~pruned]):
            inner.append((int(c << (sh + np.uint64(3))), d, int(b)))
        code, is_leaf = pc, pruned
    inner.sort(key=lambda t: (t[0], t[1]))   # preorder: by position, an ancestor before its descendants
    leaf.sort()
    data = bytes(v for _, _, b in inner for v in (b & 255, b >> 8))
    lv = np.concatenate([unmorton(np.array([c for c, _ in leaf], np.uint64)), np.array([[d] for _, d in leaf], np.int64).reshape(-1, 1)],
                        axis=1)
    return _result(len(xyz), dropped, cells, len(inner) + len(leaf), data, lv, res)


def cloud(xyz, pkg_dtype):
    """[n, 3] float32 -> rows of the package's CLOUD_DTYPE (colours are not the tree's business)."""
    xyz = np.asarray(xyz, F32).reshape(-1, 3)
    c = np.zeros(len(xyz), pkg_dtype)
    c["x"], c["y"], c["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    c["r"], c["g"], c["b"], c["a"] = 10, 20, 30, 255
    return c
