"""The cases of tests/test_gpu_train_ops.py and tests/test_train_ops_cpu.py: the smallest shapes at which the training
operators (shapemol_amd/csrc/train_ops.hip = T, shapemol_amd/csrc/sm_train.h = S) take another path, each with the line it is
there for.  Widths are small wherever a row count is the point; the production widths (308 / 128 / 128 and 20 | 128 | 32)
appear once each at a small row count.  Not a cross product: each value stands beside otherwise small, aligned dimensions.

Every seed is the first from its round number onwards for which the float64 oracle reports zero offenders of the
well-posedness conditions (`python tests/train_ops_f64.py` prints the cases whose seed has to move;
tests/test_train_ops_cpu.py asserts the cap).

Expected counts (asserted against a restatement of T:52-58 on the CPU and against the library's workspace size on the device):
  splits   partial tiles the split products really launch, real_splits (T:54-58); above 32 the 32-group reducer runs (T:37)
  blocks   64-row blocks = partials of the LayerNorm backward and of colsum (T:77, S:261); above 32 likewise
"""
from collections import namedtuple

Mlp = namedtuple("Mlp", "rows k_in hidden n_out splits blocks seed reason")
Edge = namedtuple("Edge", "n_atoms degrees k_edge k_node k_shape hidden n_out n_edges splits_e splits_n seed reason")
Attn = namedtuple("Attn", "n_atoms degrees heads dh W big_logits seed reason")
Vn = namedtuple("Vn", "n_mol atoms rows_o rows_s C training blocks seed reason")

MLP = [
    # rows
    Mlp(1, 8, 8, 8, 1, 1, 1100, "one row: every GEMM tile is one valid row of 64 (S:137 a_mvalid), LayerNorm backward block of one row (S:271)"),
    Mlp(63, 8, 8, 8, 1, 1, 1101, "one below the GEMM M tile and the LayerNorm-backward block of 64 rows (T:22, S:261)"),
    Mlp(64, 8, 8, 8, 1, 1, 1102, "exactly one M tile, one full 64-row block (T:22, S:261)"),
    Mlp(65, 8, 8, 8, 1, 2, 1104, "second M tile and second row block of one row (T:22, S:268-271)"),
    Mlp(511, 8, 8, 8, 1, 8, 1104, "last row count with one split: row_splits = 511 / 256 = 1 (T:52)"),
    Mlp(512, 8, 8, 8, 2, 8, 1105, "first row count with two splits, both chunks full (T:52, T:20)"),
    Mlp(513, 8, 8, 8, 2, 9, 1106, "two splits, chunk rounded up to 272: a ragged second chunk of 241 rows (T:20, S:125)"),
    Mlp(2048, 4, 4, 4, 8, 32, 1107, "32 row-block partials: the 8-group reducer at its limit for dgamma | dbeta | db1 and db2 (T:45-46, T:37-38)"),
    Mlp(2049, 4, 4, 4, 8, 33, 1108, "33 row-block partials: the 32-group reducer, last block one row (T:45, T:37)"),
    Mlp(8448, 4, 4, 4, 33, 132, 1109, "33 split partials through the 32-group reducer (T:37, T:128)"),
    Mlp(8449, 4, 4, 4, 32, 133, 1110, "row_splits 33 but 32 partials launched (chunk 272): real_splits < row_splits, workspace carved by real_splits, 8-group reducer at 32 (T:54-58, T:112)"),
    Mlp(65536, 4, 4, 4, 256, 1024, 1114, "the split cap: 256 partials of 256 rows (T:52)"),
    Mlp(65537, 4, 4, 4, 241, 1025, 1114, "256 splits asked, 241 launched, last chunk 257 rows (T:54-58)"),
    # k_in: the K chunk of 16 and its tail; widths that are no multiple of four take the scalar kernel
    Mlp(33, 15, 8, 8, 1, 1, 1113, "k_in 15: one K chunk with a tail, row stride not a multiple of four -> gemm_f32_kernel (T:24-27, S:56)"),
    Mlp(33, 16, 8, 8, 1, 1, 1114, "k_in 16: exactly one K chunk on the float4 kernels (T:20, S:145)"),
    Mlp(33, 17, 8, 8, 1, 1, 1115, "k_in 17: a second K chunk of one column, scalar kernel, prefetch of the next chunk (S:62-71)"),
    Mlp(33, 20, 8, 8, 1, 1, 1116, "k_in 20: second K chunk of one float4 on the float4 kernels (S:140-141, the production edge width)"),
    # hidden
    Mlp(33, 8, 1, 8, 1, 1, 1117, "hidden 1: one lane column in the LayerNorm kernels (S:233-246, S:275), one-column GEMM operands on the scalar kernel (T:24)"),
    Mlp(33, 8, 63, 8, 1, 1, 1118, "hidden 63: one below the 64-lane stride, lane 63 idle (S:233, S:275)"),
    Mlp(33, 8, 64, 8, 1, 1, 1119, "hidden 64: every lane one column, one full N tile (S:233, T:22)"),
    Mlp(33, 8, 65, 8, 1, 1, 1120, "hidden 65: lane 0 takes a second column, second N tile of one column (S:233, T:22)"),
    Mlp(33, 8, 100, 8, 1, 1, 1121, "hidden 100: a second N tile of 36 columns, lanes own one or two columns (T:22, S:233)"),
    Mlp(65, 8, 256, 8, 1, 2, 1122, "hidden 256: the LDS limit of ln_relu_bwd_kernel, 16 waves x 3 x 256 floats = 48 KB (T:12, T:63)"),
    # n_out
    Mlp(65, 8, 8, 1, 1, 2, 1123, "n_out 1: colsum with 256 row groups of one column (S:307-308), one-column GEMM"),
    Mlp(65, 8, 8, 65, 1, 2, 1124, "n_out 65: colsum with 3 groups and 61 idle threads (S:307-310), second N tile of one column, scalar kernel"),
    Mlp(65, 8, 8, 100, 1, 2, 1125, "n_out 100: a colsum group count (2) that does not divide 256, 56 idle threads (S:307-310)"),
    Mlp(130, 8, 8, 300, 1, 3, 1126, "n_out 300: colsum loops over two column blocks, 256 + 44 (S:306)"),
    # production
    Mlp(70, 308, 128, 128, 1, 2, 1127, "the production widths 308 / 128 / 128: 20 K chunks with a tail of 4 (T:20)"),
]

EDGE = [
    Edge(60, ("rand", 1, 8), 20, 128, 32, 128, 128, None, 1, 1, 1200, "the production widths 20 | 128 | 32; an atom without edges as centre, an atom that is nobody's neighbour (S:330-334 empty segments)"),
    Edge(40, ("rand", 1, 5), 4, 6, 4, 16, 8, None, 1, 1, 1201, "float4 kernels with a partial last float4 in N: dh = dpd Wd with N = 6, strides 20 (T:241, S:109-115 gemm_load4 with 2 valid lanes)"),
    Edge(40, ("rand", 1, 5), 4, 6, 0, 16, 8, None, 1, 1, 1202, "the same without a shape block: K1 = 16, k_shape == 0 skips the s products (T:186, T:243)"),
    Edge(40, ("rand", 1, 5), 7, 24, 0, 32, 8, None, 1, 1, 1203, "K1 = 55: scalar kernels, column blocks of W1 at unaligned offsets 7 and 31 (T:183, T:24-27)"),
    Edge(40, ("rand", 1, 5), 20, 6, 2, 16, 8, None, 1, 1, 1204, "K1 = 34: scalar kernels, column-block reduction into dW1 with cols 6 and 2 of ldo 34 (T:238-245, S:217)"),
    Edge(100, ("total", 511), 4, 8, 4, 8, 8, 511, 1, 1, 1205, "511 edges: the last edge count with one split (T:52, T:210)"),
    Edge(100, ("total", 512), 4, 8, 4, 8, 8, 512, 2, 1, 1206, "512 edges over 100 atoms: the edge products split in two, the node products do not (T:210, T:226 vs T:237)"),
    Edge(100, ("total", 513), 4, 8, 4, 8, 8, 513, 2, 1, 1207, "513 edges: ragged second chunk of the edge products; `part` sized by the larger of the three uses (T:159)"),
    Edge(511, ("total", 700), 4, 8, 4, 8, 8, 700, 2, 1, 1208, "511 atoms: the node products in one split while the edge products split (T:210)"),
    Edge(512, ("total", 700), 4, 8, 4, 8, 8, 700, 2, 2, 1209, "512 atoms: the node products dWd, dWs, dWi split in two (T:237-245)"),
    Edge(513, ("total", 700), 4, 8, 4, 8, 8, 700, 2, 2, 1210, "513 atoms: ragged second chunk of the node products (T:237, S:125)"),
    Edge(9, ("set", (0, 3, 1, 0)), 4, 8, 4, 8, 8, None, 1, 1, 1211, "atoms 0 and 3 have no edges as centre, atom 2 is nobody's neighbour: empty segments in both seg_rowsum launches (T:234-235)"),
    Edge(50, ("hub", 3), 4, 8, 4, 8, 8, 150, 1, 1, 1212, "every edge points to atom 0: one perm_src segment of 150 edges, 49 empty ones (T:235, S:333)"),
    Edge(2, ("total", 1), 4, 8, 4, 8, 8, 1, 1, 1, 1213, "a single edge (S:228 one row in the last workgroup, T:234 one atom without edges)"),
]

ATTN = [
    Attn(37, ("rand", 0, 8), 1, 1, 1, 0, 1300, "heads 1, dh 1, W 1: seven of eight lanes idle in both roles (S:374); 37 * 8 threads: the last wave has dead 8-lane groups (S:370)"),
    Attn(37, ("rand", 0, 8), 3, 5, 3, 0, 1301, "heads 3, dh 5, W 3: head stride no power of two (S:371-372), 888 threads"),
    Attn(37, ("rand", 0, 8), 16, 8, 8, 0, 1302, "the x2h form: heads 16, dh = W = 8, every lane live (S:374)"),
    Attn(37, ("rand", 0, 8), 16, 8, 3, 0, 1303, "the h2x form: W 3 (S:344)"),
    Attn(37, ("rand", 0, 8), 3, 8, 1, 0, 1304, "dh 8 with W 1: every lane a key component, one lane a value component (S:374, S:399-400)"),
    Attn(37, ("rand", 0, 8), 1, 5, 8, 0, 1305, "dh 5 with W 8: value lanes beyond the key lanes (S:374)"),
    Attn(41, ("set", (0, 1, 40)), 3, 5, 3, 0, 1306, "degrees 0, 1 and 40: zeros for atoms without edges (S:390), a softmax of one edge (alpha == 1, dlogit == 0), a long online pass (S:380-388)"),
    Attn(41, ("rand", 2, 6), 3, 8, 3, 8, 1307, "logits +-100 on eight atoms, the largest on the first edge (c == 1, later ex underflow) and on the last edge (the running sums rescaled by exp(-200)): both rescale branches carry weight (S:384-387)"),
]

VN = [
    # C = 1: 256 atoms per workgroup
    Vn(1, 255, 3, 4, 1, True, 1, 1400, "C 1, per 256: one atom below a full workgroup (S:445-447)"),
    Vn(1, 256, 3, 4, 1, True, 1, 1401, "C 1: exactly one workgroup, every thread an atom (S:445-447)"),
    Vn(1, 257, 3, 4, 1, True, 2, 1402, "C 1: second workgroup of one atom (S:594 n_here == 1)"),
    Vn(3, 8193, 3, 4, 1, True, 33, 1403, "C 1: 33 workgroup partials of dWf | dWd through the 32-group reducer (T:312, T:45)"),
    # C = 3: per = 85, one idle thread
    Vn(1, 84, 3, 4, 3, True, 1, 1404, "C 3, per 85: 255 of 256 threads map to (atom, channel) pairs (S:445 la >= per)"),
    Vn(1, 85, 3, 4, 3, True, 1, 1405, "C 3: exactly one workgroup of 85 atoms, thread 255 idle (S:445-447)"),
    Vn(1, 86, 3, 4, 3, True, 2, 1406, "C 3: second workgroup of one atom (S:594 n_here == 1)"),
    Vn(2, 2721, 3, 4, 3, True, 33, 1407, "C 3: 33 workgroup partials of dWf | dWd, the 32-group reducer (T:312, T:45)"),
    # C = 16
    Vn(1, 15, 3, 4, 16, True, 1, 1408, "C 16, per 16: one atom below a workgroup (S:447, S:594)"),
    Vn(1, 16, 3, 4, 16, True, 1, 1409, "C 16: exactly one workgroup of 16 atoms (S:445-447)"),
    Vn(1, 17, 3, 4, 16, True, 2, 1410, "C 16: second workgroup of one atom (S:594 n_here == 1)"),
    Vn(2, 513, 3, 4, 16, True, 33, 1411, "C 16: 33 workgroup partials of dWf | dWd, the 32-group reducer (T:312, T:45)"),
    Vn(1, 255, 3, 4, 16, True, 16, 1412, "255 atoms: one below the 256-thread stride of the batch statistics (S:485, S:577)"),
    Vn(1, 256, 3, 4, 16, True, 16, 1413, "256 atoms: every thread of the statistics kernels one atom (S:485, S:577)"),
    Vn(1, 257, 3, 4, 16, True, 17, 1414, "257 atoms: thread 0 takes a second atom (S:485)"),
    # C = 24: per = 10, 16 idle threads
    Vn(1, 9, 3, 4, 24, True, 1, 1415, "C 24, per 10: 16 idle threads per workgroup (S:445, S:525, S:595)"),
    Vn(1, 10, 3, 4, 24, True, 1, 1416, "C 24: exactly one workgroup of 10 atoms (S:445-447)"),
    Vn(1, 11, 3, 4, 24, True, 2, 1417, "C 24: second workgroup of one atom (S:594 n_here == 1)"),
    Vn(2, 321, 3, 4, 24, True, 33, 1418, "C 24: 33 workgroup partials of dWf | dWd, the 32-group reducer (T:312, T:45)"),
    # C = 64: four atoms per workgroup
    Vn(1, 3, 3, 4, 64, True, 1, 1419, "C 64, per 4: the channel limit (T:255)"),
    Vn(1, 4, 3, 4, 64, True, 1, 1420, "C 64: exactly one workgroup of four atoms (S:445-447)"),
    Vn(1, 5, 3, 4, 64, True, 2, 1421, "C 64: second workgroup of one atom (S:594 n_here == 1)"),
    Vn(2, 129, 3, 4, 64, True, 33, 1422, "C 64: 33 workgroup partials of dWf | dWd, the 32-group reducer (T:312, T:45)"),
    # operand limits and modes
    Vn(2, 40, 0, 4, 16, True, 3, 1423, "rows_o 0: no o3 operand, a null pointer for it and for do3 (T:268, T:292, S:614 rows == 1)"),
    Vn(2, 40, 3, 0, 16, True, 3, 1424, "rows_s 0: no shape operand (T:269, S:437)"),
    Vn(3, 40, 16, 32, 16, False, 3, 1425, "evaluation mode at the production widths 16 | 32 | 16: running statistics used and left alone (S:480-482, S:602)"),
    Vn(3, 40, 16, 32, 16, True, 3, 1426, "training mode at the production widths 16 | 32 | 16: Cin = 49 weights per channel in LDS (T:280, S:443)"),
    Vn(1, 2, 3, 4, 16, True, 1, 1427, "two atoms in training mode: the unbiased-variance factor n / (n - 1) = 2 in the running variance (S:494)"),
]

def zero_by_construction(kind, case):
    """Gradients that are exactly zero in exact arithmetic, so that no relative error exists: with one hidden column LayerNorm's
    output is the constant beta, nothing flows back through it (dz == 0: dx, dW1, db1) and xhat == 0 (dgamma).  Oracle and
    kernel must both give exact zeros there (S:287: dr - m1 == 0 and xr == 0)."""
    return ("dx", "dW1", "db1", "dgamma") if kind == "mlp" and case.hidden == 1 else ()


ALL = {"mlp": MLP, "edge": EDGE, "attn": ATTN, "vn": VN}


def case_id(case):
    return "-".join(str(v) if not isinstance(v, tuple) else "_".join(str(x) if not isinstance(x, tuple) else "".join(map(str, x)) for x in v)
                    for v in case[:-2])
