"""CPU checks of the dense scan's plan (scan_topk.hip make_plan), through the host-only query
irc_scan_topk_pipeline and the workspace formulas: which passes a shape takes and how many
bytes it needs, at every boundary of the rules (no device is accessed).

The expected values were recorded before make_plan was reorganised around its two
enumerations: the byte counts from the library as it was, the passes from the query added
on top of the unchanged conditions.  They pin the rules, not the code that now states them."""
import pytest

from conftest import PKG, ROOT  # noqa: F401  (import paths)

from irc_amd import _lib, retrieval

BIG = (1 << 20) + 3000

# (Q, N, D, k, dtype, single-pass min Q or None, sample, filter, chunk_docs, workspace bytes)
PLANS = [
    # Q across the one- / two-group, single-pass and GEMM-filter floors
    (1, 20000, 768, 100, "bf16", None, "none", "tile_lists", 20000, 5419264),
    (32, 20000, 768, 100, "bf16", None, "none", "tile_lists", 20000, 5419264),
    (33, 20000, 768, 100, "bf16", None, "none", "tile_lists", 20000, 10838528),
    (64, 20000, 768, 100, "bf16", None, "none", "tile_lists", 20000, 10838528),
    (65, 20000, 768, 100, "bf16", None, "tile", "tile_keys", 20000, 21677056),
    (191, 20000, 768, 100, "bf16", None, "tile", "tile_keys", 20000, 42469376),
    (192, 20000, 768, 100, "bf16", None, "tile", "gemm_keys", 20000, 42469376),
    (256, 20000, 768, 100, "bf16", None, "tile", "gemm_keys", 20000, 42469376),
    (257, 20000, 768, 100, "bf16", None, "tile", "gemm_keys", 20000, 83333120),
    (2048, 20000, 768, 100, "bf16", None, "tile", "gemm_keys", 20000, 336207872),
    # N at the GEMM filter's floor (256), the sample's, the GEMM sample's, the chunking
    (192, 1, 128, 10, "bf16", None, "none", "tile_keys", 1, 542720),
    (192, 255, 128, 10, "bf16", None, "none", "tile_keys", 255, 542720),
    (192, 256, 128, 10, "bf16", None, "none", "gemm_keys", 256, 542720),
    (192, 300, 128, 10, "bf16", None, "none", "gemm_keys", 300, 1083392),
    (192, 4099, 128, 10, "bf16", None, "tile", "gemm_keys", 4099, 9193472),
    (192, 20000, 128, 10, "bf16", None, "tile", "gemm_keys", 20000, 42600448),
    (192, 50000, 128, 10, "bf16", None, "gemm", "gemm_keys", 50000, 103565312),
    (192, 600000, 128, 10, "bf16", None, "gemm", "gemm_keys", 600000, 1243916288),
    (192, BIG, 128, 10, "bf16", None, "gemm", "gemm_keys", 525824, 1092146176),
    (192, 5000000, 128, 10, "bf16", None, "gemm", "gemm_keys", 1000192, 2084492800),
    (1, 1, 768, 10, "bf16", None, "none", "tile_lists", 1, 69888),
    (1, 255, 768, 10, "bf16", None, "none", "tile_lists", 255, 69888),
    (1, 256, 768, 10, "bf16", None, "none", "tile_lists", 256, 69888),
    (1, 300, 768, 10, "bf16", None, "none", "tile_lists", 300, 139520),
    (1, 4099, 768, 10, "bf16", None, "none", "tile_lists", 4099, 1184000),
    (1, 20000, 768, 10, "bf16", None, "none", "tile_lists", 20000, 5419264),
    (1, 50000, 768, 10, "bf16", None, "none", "tile_lists", 50000, 12960000),
    (1, 600000, 768, 10, "bf16", None, "none", "tile_lists", 600000, 155320576),
    (1, BIG, 768, 10, "bf16", None, "none", "tile_lists", BIG, 270663936),
    (1, 5000000, 768, 10, "bf16", None, "none", "tile_lists", 5000000, 1281491200),
    (65, 1, 512, 100, "bf16", None, "none", "tile_keys", 1, 271360),
    (65, 255, 512, 100, "bf16", None, "none", "tile_keys", 255, 271360),
    (65, 256, 512, 100, "bf16", None, "none", "tile_keys", 256, 271360),
    (65, 300, 512, 100, "bf16", None, "none", "tile_keys", 300, 541696),
    (65, 4099, 512, 100, "bf16", None, "none", "tile_keys", 4099, 4596736),
    (65, 20000, 512, 100, "bf16", None, "tile", "tile_keys", 20000, 21455872),
    (65, 50000, 512, 100, "bf16", None, "tile", "tile_keys", 50000, 51610624),
    (65, 600000, 512, 100, "bf16", None, "tile", "tile_keys", 600000, 621020160),
    (65, BIG, 512, 100, "bf16", None, "tile", "tile_keys", BIG, 1082393600),
    (65, 5000000, 512, 100, "bf16", None, "tile", "tile_keys", 5000000, 5125702656),
    # k across the lists' limit (256), the selects' two builds (512) and the sample's 4 k
    (32, 20000, 768, 1, "bf16", None, "none", "tile_lists", 20000, 5419264),
    (32, 20000, 768, 4, "bf16", None, "none", "tile_lists", 20000, 5419264),
    (32, 20000, 768, 10, "bf16", None, "none", "tile_lists", 20000, 5419264),
    (32, 20000, 768, 256, "bf16", None, "none", "tile_lists", 20000, 5419264),
    (32, 20000, 768, 257, "bf16", None, "tile", "tile_keys", 20000, 5419264),
    (32, 20000, 768, 512, "bf16", None, "none", "tile_keys", 20000, 5419264),
    (32, 20000, 768, 513, "bf16", None, "none", "tile_keys", 20000, 5419264),
    (32, 20000, 768, 1024, "bf16", None, "none", "tile_keys", 20000, 5419264),
    (192, 600000, 128, 1, "bf16", None, "gemm", "gemm_keys", 600000, 1243916288),
    (192, 600000, 128, 4, "bf16", None, "gemm", "gemm_keys", 600000, 1243916288),
    (192, 600000, 128, 100, "bf16", None, "gemm", "gemm_keys", 600000, 1243916288),
    (192, 600000, 128, 256, "bf16", None, "tile", "gemm_keys", 600000, 1243916288),
    (192, 600000, 128, 257, "bf16", None, "tile", "gemm_keys", 600000, 1243916288),
    (192, 600000, 128, 512, "bf16", None, "tile", "gemm_keys", 600000, 1243916288),
    (192, 600000, 128, 513, "bf16", None, "tile", "gemm_keys", 600000, 1243916288),
    (192, 600000, 128, 1024, "bf16", None, "tile", "gemm_keys", 600000, 1243916288),
    (65, 50000, 1024, 1, "bf16", None, "tile", "tile_keys", 50000, 51840000),
    (65, 50000, 1024, 4, "bf16", None, "tile", "tile_keys", 50000, 51840000),
    (65, 50000, 1024, 10, "bf16", None, "tile", "tile_keys", 50000, 51840000),
    (65, 50000, 1024, 100, "bf16", None, "tile", "tile_keys", 50000, 51840000),
    (65, 50000, 1024, 256, "bf16", None, "tile", "tile_keys", 50000, 51840000),
    (65, 50000, 1024, 257, "bf16", None, "tile", "tile_keys", 50000, 51840000),
    (65, 50000, 1024, 512, "bf16", None, "tile", "tile_keys", 50000, 51840000),
    (65, 50000, 1024, 513, "bf16", None, "tile", "tile_keys", 50000, 51840000),
    (65, 50000, 1024, 1024, "bf16", None, "none", "tile_keys", 50000, 51840000),
    # D: one and two k-slices, the four-slice promotion of the lists
    (33, 4099, 64, 10, "bf16", None, "none", "tile_lists", 4099, 2298368),
    (33, 4099, 512, 10, "bf16", None, "none", "tile_lists", 4099, 2298368),
    (33, 4099, 768, 10, "bf16", None, "none", "tile_lists", 4099, 2368000),
    (33, 4099, 1024, 10, "bf16", None, "none", "tile_lists", 4099, 2368000),
    (256, 600000, 64, 100, "bf16", None, "gemm", "gemm_keys", 600000, 1243916288),
    (256, 600000, 512, 100, "bf16", None, "gemm", "gemm_keys", 600000, 1243916288),
    (256, 600000, 768, 100, "bf16", None, "gemm", "gemm_keys", 600000, 1235527680),
    (256, 600000, 1024, 100, "bf16", None, "gemm", "gemm_keys", 600000, 1235527680),
    # e4m3: never on the GEMM kernel at D = 64 (128-byte K-tiles), never chunked there
    (192, 20000, 64, 4, "e4m3", None, "tile", "tile_keys", 20000, 42600448),
    (192, 20000, 128, 4, "e4m3", None, "gemm", "gemm_keys", 20000, 42600448),
    (192, 20000, 128, 100, "e4m3", None, "tile", "gemm_keys", 20000, 42600448),
    (192, 300, 128, 10, "e4m3", None, "none", "gemm_keys", 300, 1083392),
    (1, 20000, 64, 10, "e4m3", None, "tile", "tile_keys", 20000, 5339392),
    (64, 50000, 1024, 100, "e4m3", None, "none", "tile_lists", 50000, 25920000),
    (2048, 5000000, 512, 100, "e4m3", None, "gemm", "gemm_keys", 1000192, 16452427776),
    (2048, 5000000, 64, 100, "e4m3", None, "tile", "tile_keys", 5000000, 81940987904),
    (256, BIG, 1024, 1024, "e4m3", None, "tile", "gemm_keys", 525824, 1090527232),
    # chunked: the survivor workspace over its cap, more tiles than the select's table
    (2048, 5000000, 768, 100, "bf16", None, "gemm", "gemm_keys", 1000192, 16435650560),
    (2048, BIG, 128, 10, "bf16", None, "gemm", "gemm_keys", 525824, 8640823296),
    # the single-pass GEMM filter switched on from Q = 65
    (100, 4099, 128, 10, "bf16", 65, "none", "gemm_lists", 4099, 4596736),
    (65, 4099, 128, 10, "bf16", 65, "none", "gemm_lists", 4099, 4596736),
    (64, 4099, 128, 10, "bf16", 65, "none", "tile_lists", 4099, 2298368),
    (256, 20000, 768, 100, "bf16", 65, "none", "gemm_lists", 20000, 42469376),
    (257, 20000, 768, 100, "bf16", 65, "tile", "gemm_keys", 20000, 83333120),
    (100, 4099, 128, 257, "bf16", 65, "none", "tile_keys", 4099, 4596736),
    (100, 255, 128, 10, "bf16", 65, "none", "tile_keys", 255, 271360),
    (100, 600000, 128, 10, "bf16", 65, "tile", "tile_keys", 600000, 618628096),
    (100, 4099, 64, 10, "e4m3", 65, "tile", "tile_keys", 4099, 4596736),
    (100, 4099, 128, 10, "e4m3", 65, "none", "gemm_lists", 4099, 4596736),
    # tests/test_scan_gpu.py: the sorted corpus at k = 100 (56 sample list keys < 4 k) and
    # k = 10 (52 >= 4 k), and one shape per pair
    (300, 50000, 128, 100, "bf16", None, "tile", "gemm_keys", 50000, 206442496),
    (300, 50000, 128, 10, "bf16", None, "gemm", "gemm_keys", 50000, 206442496),
    (65, 300, 64, 10, "bf16", None, "none", "tile_keys", 300, 541696),
    (65, 20000, 128, 4, "bf16", None, "tile", "tile_keys", 20000, 21357568),
    (192, 20000, 128, 100, "bf16", None, "tile", "gemm_keys", 20000, 42600448),
    (192, 20000, 128, 4, "bf16", None, "gemm", "gemm_keys", 20000, 42600448),
]

REACHABLE = {("none", "tile_lists"), ("none", "gemm_lists"), ("none", "tile_keys"),
             ("tile", "tile_keys"), ("none", "gemm_keys"), ("tile", "gemm_keys"),
             ("gemm", "gemm_keys")}


class _min_q:
    """The single-pass GEMM filter's floor set inside a block (None: left as it is)."""

    def __init__(self, q):
        self.q = q

    def __enter__(self):
        if self.q is not None:
            self.prev = retrieval.set_single_pass_min_q(self.q)

    def __exit__(self, *exc):
        if self.q is not None:
            retrieval.set_single_pass_min_q(self.prev)


def test_entry_is_exported_and_bound():
    lib = _lib.load()
    assert lib.irc_abi_version() == 2  # the addition is additive
    assert "irc_scan_topk_pipeline" in _lib.SIGNATURES
    with open(f"{ROOT}/include/irc.h") as f:
        header = f.read()
    assert "int irc_scan_topk_pipeline(" in header
    for i, name in enumerate(retrieval.SCAN_SAMPLES):
        assert f"#define IRC_SCAN_SAMPLE_{name.upper()} {i} " in header
    for i, name in enumerate(retrieval.SCAN_FILTERS):
        assert f"#define IRC_SCAN_FILTER_{name.upper()} {i} " in header


def test_table_covers_every_reachable_pair_and_chunking():
    assert {(r[6], r[7]) for r in PLANS} == REACHABLE
    assert any(r[8] < r[1] for r in PLANS)


@pytest.mark.parametrize("row", PLANS, ids=[
    "-".join(str(x) for x in r[:5]) + ("" if r[5] is None else f"-sp{r[5]}") for r in PLANS])
def test_plan(row):
    Q, N, D, k, dtype, min_q, sample, filt, chunk, nbytes = row
    ws = "irc_scan_topk_fp8_workspace" if dtype == "e4m3" else "irc_scan_topk_workspace"
    with _min_q(min_q):
        assert retrieval.scan_pipeline(Q, N, D, k, dtype) == (sample, filt, chunk)
        assert int(_lib.fn(ws)(Q, N, D, k)) == nbytes


def test_setter_is_restored():
    prev = retrieval.set_single_pass_min_q(1 << 30)
    assert retrieval.set_single_pass_min_q(prev) == 1 << 30
    assert prev == 1 << 30  # the default: off


@pytest.mark.parametrize("kw,msg", [
    (dict(N=-1), "negative size"), (dict(Q=-1), "negative size"), (dict(k=0), "k=0"),
    (dict(k=1025), "k=1025"), (dict(D=100), "unsupported D=100"),
    (dict(Q=1 << 24), "Q too large"), (dict(N=(1 << 31) - 64), "shard too large"),
])
def test_invalid_sizes_are_rejected_as_the_scan_rejects_them(kw, msg):
    args = dict(Q=4, N=1000, D=128, k=5)
    args.update(kw)
    with pytest.raises(_lib.IRCError, match=msg):
        retrieval.scan_pipeline(**args)
    with pytest.raises(ValueError):
        retrieval.scan_pipeline(4, 1000, 128, 5, dtype="fp16")
