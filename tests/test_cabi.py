"""The C-ABI library loads on a CPU-only host and exports every symbol include/marl_hip.h declares;
the ctypes table lists exactly those symbols.  No compute is called."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "marl_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(marl_[a-z0-9_]+)\s*\(", txt)))


def exported_symbols(path):
    """names of the defined symbols in the dynamic symbol table of an ELF64 little-endian shared object"""
    blob = open(path, "rb").read()
    assert blob[:6] == b"\x7fELF\x02\x01", "not a 64-bit little-endian ELF file"
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", blob, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, sh_type, _, _, off, size, link, _, _, entsize in secs:
        if sh_type == 11:                                   # SHT_DYNSYM; its sh_link is the string table
            strtab = secs[link][4]
            for k in range(size // entsize):
                st_name, _, _, st_shndx = struct.unpack_from("<IBBH", blob, off + k * entsize)
                if st_shndx != 0:                           # defined here, not imported
                    names.add(blob[strtab + st_name:blob.index(b"\0", strtab + st_name)].decode())
    return names


# exported with C linkage but no part of the C ABI: the accessor of the experiment-switch table that the library's own objects
# share (csrc/common.h declares it, optim.hip defines it; it returns a C++ struct the public header does not know).  Callers use
# marl_experiment_set / marl_experiment_get.
LIBRARY_INTERNAL = {"marl_switches"}


def test_library_exports_every_declared_symbol():
    from marl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 25
    for s in syms:
        assert hasattr(lib, s), "missing export " + s
    assert set(_lib.SIGNATURES) == set(syms), set(_lib.SIGNATURES) ^ set(syms)
    # ... and the other way round: nothing the library exports under the project's prefix is without a signature
    exported = {s for s in exported_symbols(_lib.LIB_PATH) if s.startswith("marl_")}
    assert LIBRARY_INTERNAL <= exported                        # (the exception list cannot go stale)
    assert exported - LIBRARY_INTERNAL == set(_lib.SIGNATURES), exported ^ set(_lib.SIGNATURES)
    _lib.load()
    assert b"gfx950" in _lib.load().marl_hip_version()


def _host_cc():
    """the host C compiler: cc, else the clang that ships beside hipcc"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    beside = os.path.dirname(os.path.realpath(hipcc))
    for c in ("cc", os.path.join(beside, "clang"), os.path.join(beside, "amdclang"),
              os.path.join(beside, "..", "lib", "llvm", "bin", "clang")):
        if shutil.which(c):
            return shutil.which(c)
    return None


def test_struct_layouts_match_the_host_c_compiler(tmp_path):
    """sizeof / offsetof of every struct of the header as the C compiler lays it out, against the ctypes classes _lib derives
    from the same header.  The C side never passes through _lib's type mapping: a reader that takes a `long` for an `int` (or drops
    a field) shows here as a moved offset."""
    from marl_amd import _lib
    cc = _host_cc()
    assert cc is not None, "no host C compiler (cc, or clang beside hipcc): build() needs one as well"
    assert len(_lib.STRUCTS) >= 18 and _lib.STRUCTS["marl_src_t"] is _lib.MarlSrc
    assert _lib.STRUCTS["marl_maic_infer_grads_t"] is _lib.MarlMaicInferGrads and _lib.MarlG2anetWeights.__name__ == "MarlG2anetWeights"
    prog = ["#include <stdio.h>", "#include <stddef.h>", '#include "marl_hip.h"', "int main(void) {"]
    want = {}
    for cname, cls in _lib.STRUCTS.items():
        prog.append('  printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        want[cname] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            prog.append('  printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, field, cname, field))
            want[cname + "." + field] = getattr(cls, field).offset
    prog += ["  return 0;", "}", ""]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert got == want
    assert got["marl_src_t"] == 144 and got["marl_src_t.emap0"] == 136          # (a 64-bit host: what the library is built for)


# the entries that take the episode record, and the loose device arrays each keeps beside it (stream not counted)
RECORD_ENTRIES = {"marl_synth_observe": (), "marl_synth_step": ("act", "alive_next"),
                  "marl_synth_fused_step": ("q",), "marl_synth_fused_step_sample": ("q",),
                  "marl_synth_rollout": ("eps", "h_out", "stats"), "marl_synth_rollout_sample": ("eps", "h_out", "stats"),
                  "marl_synth_rollout_x6": ("eps", "h_out", "stats"),
                  "marl_battle_reset": ("units",), "marl_battle_step": ("act", "units", "alive_next"),
                  "marl_battle_fused_step": ("q", "units"), "marl_battle_fused_step_sample": ("q", "units"),
                  "marl_battle_rollout": ("units", "h_out", "stats"), "marl_battle_rollout_sample": ("units", "h_out", "stats")}


def test_the_episode_record_travels_as_one_struct():
    from marl_amd import _lib
    P, I, L, F, U = _lib.P, _lib.I, _lib.L, _lib.F, _lib.U
    rec = _lib.STRUCTS["marl_record_t"]
    assert rec is _lib.MarlRecord
    assert rec._fields_ == [("obs", P), ("state", P), ("avail", P), ("state_ld", L), ("u", P), ("r", P), ("term", P), ("padded", P),
                            ("length", P), ("won", P), ("E", I), ("T", I), ("N", I), ("O", I), ("S", I), ("A", I)]
    assert len(RECORD_ENTRIES) == 13
    for name, loose in RECORD_ENTRIES.items():
        res, args = _lib.SIGNATURES[name]
        assert res is I and args.count(ctypes.POINTER(rec)) == 1, name
        assert args[-1] is P and args[:-1].count(P) <= len(loose), (name, "loose pointers beside the record (and the stream)")
    # the three neighbours that keep their loose lists
    assert _lib.SIGNATURES["marl_synth_lengths"] == (I, [U, I, I, P, P, I, I, P])
    assert _lib.SIGNATURES["marl_select_actions"] == (I, [P, P, L, P, F, U, I, P, I, P, L, I, I, I, P])
    assert _lib.SIGNATURES["marl_replay_gather"] == (I, [P, I, I, I, I] + [P] * 18)


DEMO_HEADER = """/* a comment
 * over two lines */
#ifndef DEMO_H
#define DEMO_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef struct {
  const float *a, *b;   /* two declarators on one line */
  long long* n;
  long x, y; int k;
} marl_demo_t;
#define MARL_DEMO_FLAG 1   /* a constant */
int marl_demo(const marl_demo_t* w, marl_demo_t* g, const char* name, const long long* idx, unsigned k, size_t n,
              double d, float f, long m, const void* y, void* stream);
size_t marl_demo_bytes(int n);
const char* marl_demo_version(void);
#ifdef __cplusplus
}
#endif
#endif
"""


def test_header_reader_reads_the_headers_grammar_and_nothing_else():
    """parse_header on a small header: the positive cases (several declarators on a line, `long long*`, struct pointers, const char*),
    then one foreign construct at a time - each must raise and name the line it stands on, never guess."""
    from marl_amd import _lib
    P, I, L, F, U, SZ, D = _lib.P, _lib.I, _lib.L, _lib.F, _lib.U, _lib.SZ, _lib.D
    structs, sigs = _lib.parse_header(DEMO_HEADER)
    demo = structs["marl_demo_t"]
    assert list(structs) == ["marl_demo_t"] and demo.__name__ == "MarlDemo" and issubclass(demo, ctypes.Structure)
    assert demo._fields_ == [("a", P), ("b", P), ("n", P), ("x", L), ("y", L), ("k", I)]
    assert sigs == {"marl_demo": (I, [ctypes.POINTER(demo), ctypes.POINTER(demo), ctypes.c_char_p, P, U, SZ, D, F, L, P, P]),
                    "marl_demo_bytes": (SZ, [I]), "marl_demo_version": (ctypes.c_char_p, [])}

    def refused(old, new, line, word):
        assert DEMO_HEADER.count(old) == 1
        with pytest.raises(_lib.MarlHipError, match=r"line %d: .*%s" % (line, word)):
            _lib.parse_header(DEMO_HEADER.replace(old, new))
    refused("long x, y;", "short x, y;", 12, "short")                                      # an unknown scalar type: a field ...
    refused("unsigned k, size_t n", "unsigned k, uint64_t n", 15, "uint64_t")              # ... and an argument
    refused("marl_demo_t* g,", "marl_demo_t g,", 15, "marl_demo_t g")                      # a struct by value
    refused("size_t marl_demo_bytes(int n);", "size_t marl_demo_bytes(int (*cb)(int), int n);", 17, "marl_demo_bytes")   # cannot be split
    refused("size_t marl_demo_bytes(int n);", "size_t marl_demo_bytes(int n[4]);", 17, r"n\[4\]")
    refused("size_t marl_demo_bytes(int n);", "size_t marl_demo_bytes(int);", 17, "int")          # (every argument is named)
    refused("const char* marl_demo_version", "char* marl_demo_version", 18, "char")
    refused("float f, long m", "float** f, long m", 16, "float")
    refused("const void* y", "const marl_other_t* y", 16, "marl_other_t")                   # a struct the header does not define
    refused("#define MARL_DEMO_FLAG 1 ", "#define MARL_DEMO_FLAG \\\n 1 ", 14, "MARL_DEMO_FLAG")
    refused("} marl_demo_t;", "} demo_t;", 9, "typedef")


def test_header_is_found_beside_the_package():
    from marl_amd import _lib
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "marl_hip.h"))
    missing = os.path.join(ROOT, "include", "no_such_header.h")
    old, _lib.HEADER_PATH = _lib.HEADER_PATH, missing
    try:
        with pytest.raises(_lib.MarlHipError, match="not found"):
            _lib._read_header()
    finally:
        _lib.HEADER_PATH = old


def test_product_fails_loudly_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from oracle import seeded
    from marl_amd.controller.share_params import SharedMAC
    from marl_amd.algorithm.q_learner import QLearner
    from marl_amd.env.synthetic_smac import SyntheticSMACEnv
    args = seeded.make_args("2s3z", "qmix", episode_limit=4)
    mac = SharedMAC(args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        QLearner(mac, args)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mac.init_hidden(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SyntheticSMACEnv(4, 5, 80, 120, 11, 4)


def test_product_never_imports_oracle():
    for dp, _, fs in os.walk(os.path.join(ROOT, "marl_amd")):
        for f in fs:
            if f.endswith(".py"):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dp, f)


def _src_cpu(k):
    """a marl_src_t describing a dense (rows, k) input with 16-byte aligned rows (widths only: no device memory is touched)"""
    from marl_amd._lib import MarlSrc
    s = MarlSrc()
    s.p0, s.ld0, s.k0 = 4096, (k + 3) // 4 * 4, k
    return s


def test_split_kernel_capability_predicates():
    """The *_supported entry points of the bf16x6 kernels are host functions (no GPU): which agent shapes the split unroll and the
    split BPTT cover - the three map sizes of BASELINE's configurations - and what they leave to the fp32 kernels."""
    from marl_amd import _lib
    lib = _lib.load()
    fwd = lambda B, T, N, O, A, la=1, ru=1: lib.marl_agent_unroll_x6_supported(B, T, N, O, A, la, ru)
    bwd = lambda B, T, N, A, sparse=1: lib.marl_agent_unroll_bwd_x6_supported(B, T, N, A, sparse)
    assert fwd(512, 120, 5, 80, 11) == 1            # 2s3z: 96 input columns, three fc1 chunks
    assert fwd(512, 150, 8, 128, 14) == 1           # 3s5z: 150 columns, five chunks
    assert fwd(1024, 120, 10, 176, 18) == 1         # MMM2: 204 columns, seven chunks, two action tiles
    assert fwd(512, 3, 5, 80, 11) == 0              # T < 4: no pipeline to fill - the fp32 kernels
    assert fwd(512, 120, 5, 80, 18) == 0            # more than 16 actions on a narrow input: one action tile only
    assert fwd(512, 120, 10, 240, 18) == 0          # wider than 224 input columns
    assert fwd(512, 120, 5, 84, 11) == 0            # observation width not a multiple of 8
    assert fwd(512, 120, 5, 192, 11) == 1 and fwd(512, 120, 5, 200, 11) == 0      # O <= 192: three prefetch registers per thread of one team
    assert fwd(512, 120, 8, 128, 16) == 1 and fwd(512, 120, 8, 128, 17) == 0      # 152 / 153 input columns: one action tile up to 160 columns
    assert fwd(512, 120, 10, 176, 32) == 1 and fwd(512, 120, 10, 176, 33) == 0    # wider than 160: two action tiles, 32 actions at most
    # the split whole-rollout kernel: 2s3z-, 3s5z- and MMM2-sized agents (<= 224 input columns; <= 16 actions up to 160 columns, <= 32
    # beyond: two action tiles; whole environments in at most five - wide inputs: four / three - row tiles of 16 rows, an environment's
    # agents on one wave)
    rx6 = lib.marl_synth_rollout_x6_supported
    assert rx6(5, 80, 11) == 1 and rx6(8, 128, 14) == 1 and rx6(2, 4, 3) == 1 and rx6(49, 40, 5) == 1 and rx6(33, 100, 5) == 1
    assert rx6(10, 176, 18) == 1 and rx6(4, 180, 32) == 1 and rx6(4, 180, 33) == 0 and rx6(10, 200, 18) == 0
    assert rx6(5, 80, 17) == 0 and rx6(5, 82, 11) == 0 and rx6(65, 40, 5) == 0 and rx6(64, 40, 5) == 1 and rx6(49, 176, 18) == 0
    # the flag-aware predicate: the same with both flags on; the flags decide the input width and with it the chunk count - two action
    # tiles only beyond 160 columns of the REAL row
    rx6f = lib.marl_synth_rollout_x6_supported_flags
    for shp in ((5, 80, 11), (8, 128, 14), (2, 4, 3), (49, 40, 5), (33, 100, 5), (10, 176, 18), (4, 180, 32), (4, 180, 33), (10, 200, 18),
                (5, 80, 17), (5, 82, 11), (65, 40, 5), (64, 40, 5), (49, 176, 18), (4, 140, 20)):
        assert rx6f(*shp, 1, 1) == rx6(*shp), shp
    assert rx6f(4, 140, 20, 0, 1) == 0              # 144 columns without the last action: five chunks, one action tile
    assert rx6f(4, 140, 20, 1, 1) == 1              # 164 columns: seven chunks, two action tiles
    assert rx6f(10, 176, 18, 0, 1) == 1             # MMM2 without the last action: 186 columns, still seven chunks
    assert rx6f(10, 176, 18, 1, 0) == 1 and rx6f(10, 176, 18, 0, 0) == 1 and rx6f(10, 140, 18, 0, 0) == 0
    # ... and how a batch runs: the round-5 decomposition while it holds one row tile per workgroup, the round-6 one (up to five tiles)
    # beyond - (decomposition, workgroups, row tiles, environments per workgroup, fc1 chunks)
    import ctypes
    def plan(E, N, O, A):
        out = (ctypes.c_int * 5)()
        assert lib.marl_synth_rollout_x6_plan(E, N, O, A, 1, 1, out) == 0
        return tuple(out)
    assert plan(512, 5, 80, 11) == (1, 256, 1, 2, 3) and plan(768, 5, 80, 11) == (1, 256, 1, 3, 3) and plan(1024, 5, 80, 11) == (2, 256, 2, 4, 3)
    assert plan(2304, 5, 80, 11) == (2, 256, 3, 9, 3)
    assert plan(4096, 5, 80, 11) == (2, 256, 5, 16, 3) and plan(8192, 5, 80, 11) == (2, 512, 5, 16, 3)
    assert plan(2048, 8, 128, 14) == (2, 256, 4, 8, 5) and plan(100, 49, 40, 5) == (2, 100, 4, 1, 3)
    assert plan(1024, 10, 176, 18) == (2, 256, 3, 4, 7) and plan(2048, 10, 176, 18) == (2, 512, 3, 4, 7)      # MMM2: three tiles at most
    assert lib.marl_synth_rollout_x6_plan(512, 10, 200, 18, 1, 1, (ctypes.c_int * 5)()) != 0
    assert lib.marl_synth_rollout_x6_plan(2048, 4, 140, 20, 0, 1, (ctypes.c_int * 5)()) != 0      # (the flag-aware predicate)
    out = (ctypes.c_int * 5)()
    assert lib.marl_synth_rollout_x6_plan(2048, 10, 176, 18, 0, 1, out) == 0 and tuple(out) == (2, 512, 3, 4, 7)
    # the fused-head split pair: the padded input width must leave a free column in its last 64-column block
    m3 = lambda k, n3=1: lib.marl_mlp3_x6_supported(__import__("ctypes").byref(_src_cpu(k)), k, 64, 64, n3, 10)
    assert m3(112) == 1 and m3(120) == 1 and m3(175) == 1 and m3(188) == 1
    assert m3(191) == 0                             # a dense input of 191 columns is padded to 192 by the kernels: no free column
    assert m3(128) == 0 and m3(192) == 0 and m3(64) == 0 and m3(120, 17) == 0
    assert bwd(512, 120, 5, 11) == 1 and bwd(1024, 120, 10, 18) == 1 and bwd(512, 150, 8, 14) == 1
    assert bwd(512, 120, 5, 11, 0) == 0             # a dense dq: the fp32 kernels
    assert bwd(512, 2, 5, 11) == 0 and bwd(512, 120, 5, 40) == 0
    # workspace: one slab per workgroup - one row tile (16 rows) per workgroup up to 256 tiles; beyond that two-tile workgroups in
    # full rounds of 256, and what is left as one-tile workgroups when that is at most one round, else two-tile workgroups throughout
    slab = 4 * (2 * 192 * 64 + 11 * 64 + 2 * 192 + 11)
    assert lib.marl_agent_bwd_x6_workspace(512, 5, 11) == (512 * 5 // 16) * slab
    assert lib.marl_agent_bwd_x6_workspace(4096, 5, 11) == (512 + 256) * slab          # 1280 tiles = 2 x 512 + 256
    assert lib.marl_agent_bwd_x6_workspace(2048, 5, 11) == (256 + 128) * slab          # 640 tiles = 512 + 128
    assert lib.marl_agent_bwd_x6_workspace(3000, 5, 11) == 469 * slab                  # 938 tiles = 512 + 426: two-tile workgroups throughout
    assert lib.marl_agent_bwd_x6_workspace(1024, 5, 11) == 160 * slab                  # 320 tiles: less than one full round of two-tile workgroups


def test_forward_unroll_plan_query_at_the_learners_sizes():
    """marl_agent_unroll_fwd_plan (a host function, no GPU: the planner the launch itself calls) at the sizes the learner runs -
    (family 0 fp32 pipelined / 1 fp32 multi-tile / 2 split / 3 split round-6, row tiles per workgroup, workgroups, workgroups holding
    that many tiles, action tiles, fc1 chunks, input path 0 element / 1 vector / 2 half-tile / 3 W2L, reads gi_in)."""
    from marl_amd import ops
    q = ops.agent_unroll_fwd_plan
    save, plain, cont = dict(saved=True, gi_out=True), dict(hs=False), dict(gi_in=True, hs=False)
    s2 = lambda x6, E, cu, kw: q(x6, E, 120, 5, 80, 11, cu_budget=cu, **kw)
    # 2s3z, 512 environments = 160 row tiles: the pair schedule (128 CUs) packs two tiles per workgroup, the whole chip one (pipelined)
    assert s2(0, 512, 128, save) == (1, 2, 80, 80, 1, 6, 1, 0) and s2(0, 512, 128, cont) == (1, 2, 80, 80, 1, 6, 1, 1)
    assert s2(0, 512, 0, save) == s2(0, 512, 0, plain) == (0, 1, 160, 160, 1, 6, 1, 0) and s2(0, 512, 0, cont) == (0, 1, 160, 160, 1, 6, 1, 1)
    assert s2(1, 512, 128, save) == (2, 2, 80, 80, 1, 3, 1, 0) and s2(1, 512, 0, save) == s2(1, 512, 0, plain) == (2, 1, 160, 160, 1, 3, 1, 0)
    assert s2(1, 512, 0, cont) == (2, 1, 160, 160, 1, 3, 1, 1)
    # 4096 environments = 1280 tiles: fp32 at the six tiles LDS allows (half-tile prefetch when nothing is saved) / five on the whole
    # chip; the split kernel in rounds - 2 x 256 two-tile + 256 one-tile workgroups - and its plain unroll on round 6 at five tiles
    assert s2(0, 4096, 128, save) == (1, 6, 214, 213, 1, 6, 1, 0) and s2(0, 4096, 128, plain) == (1, 6, 214, 213, 1, 6, 2, 0)
    assert s2(0, 4096, 0, save) == (1, 5, 256, 256, 1, 6, 1, 0) and s2(0, 4096, 0, cont) == (1, 5, 256, 256, 1, 6, 1, 1)
    assert s2(1, 4096, 128, save) == (2, 2, 640, 640, 1, 3, 1, 0) and s2(1, 4096, 0, save) == (2, 2, 768, 512, 1, 3, 1, 0)
    assert s2(1, 4096, 0, plain) == (3, 5, 256, 256, 1, 3, 1, 0) and s2(1, 4096, 0, cont) == (2, 2, 768, 512, 1, 3, 1, 1)
    assert s2(1, 4096, 0, dict(hs=True)) == (2, 2, 768, 512, 1, 3, 1, 0)          # (hidden states wanted: not the round-6 kernel)
    # MMM2 at 1024 environments = 640 tiles: saving on W2L at three tiles alone on the chip, two beside the target unroll
    mm = lambda x6, cu, kw: q(x6, 1024, 120, 10, 176, 18, cu_budget=cu, **kw)
    assert mm(0, 0, save) == (1, 3, 214, 213, 2, 13, 3, 0) and mm(0, 128, save) == (1, 2, 320, 320, 2, 13, 1, 0)
    assert mm(0, 0, plain) == (1, 3, 214, 213, 2, 13, 2, 0) and mm(0, 128, plain) == (1, 4, 160, 160, 2, 13, 2, 0)
    assert mm(0, 0, cont) == (1, 3, 214, 213, 2, 13, 1, 1)
    assert mm(1, 0, save) == mm(1, 128, save) == mm(1, 0, plain) == (2, 1, 640, 640, 2, 7, 1, 0) and mm(1, 0, cont) == (2, 1, 640, 640, 2, 7, 1, 1)
    # the round-6 threshold: more than 512 tiles, whole chip, no hidden states, h0 / h_last 16-byte aligned
    r6 = lambda rows, **kw: q(1, rows, 4, 1, 48, 11, **dict(dict(hs=False), **kw))
    assert r6(8192) == (2, 2, 256, 256, 1, 3, 1, 0) and r6(8193) == (3, 3, 171, 171, 1, 3, 1, 0)
    assert r6(8193, hs=True) == r6(8193, h_aligned=False) == r6(8193, cu_budget=128) == (2, 2, 257, 256, 1, 3, 1, 0)
    assert bool(lib_r6(8193)) and not lib_r6(8192)
    # refusals: what either entry point returns hipErrorInvalidValue for
    assert q(0, 512, 120, 5, 80, 33) is None and q(1, 512, 120, 5, 80, 11, obs_aligned=False) is None and q(1, 512, 3, 5, 80, 11) is None
    assert q(0, 512, 120, 5, 80, 11, obs_aligned=False) == (1, 1, 160, 160, 1, 6, 0, 0)          # (fp32: element-wise instead)


def lib_r6(rows):
    from marl_amd import ops
    return ops.agent_unroll_x6_plain_r6(rows, 4, 1, 48, 11)


def test_qtran_row_kernel_predicates_and_workspace():
    """Host functions of the QTRAN row-level kernels (no GPU): which state widths / encoder widths they cover, and the slab
    workspace the row-gradient kernel asks for (256 workgroups x [64 x 16 ceil(S/16) | 64 x AEP | 64 x 64 | AEP x AEP | 256])."""
    from marl_amd import _lib
    lib = _lib.load()
    sp, wg, ws = lib.marl_qtran_state_parts_supported, lib.marl_qtran_wgrad_rows_supported, lib.marl_qtran_wgrad_rows_workspace
    assert sp(216) and sp(120) and sp(322) and sp(1) and sp(384)          # (S % 4 != 0: padded rows, checked per call)
    assert not sp(0) and not sp(385)
    assert wg(216, 78) and wg(120, 64) and wg(384, 80) and wg(4, 64)
    assert not wg(322, 74) and not wg(388, 78) and not wg(216, 81) and not wg(216, 48)
    for S, AE in ((216, 78), (120, 64), (384, 80)):
        aep, ts = (AE + 15) // 16 * 16, (S + 15) // 16
        assert ws(S, AE) == 256 * (64 * 16 * ts + 64 * aep + 64 * 64 + aep * aep + 256) * 4


def test_qtran_plan_query():
    """marl_qtran_plan (a host function, no GPU: the planners the launches of csrc/qtran_fused.hip themselves decide with) either
    side of every step of the launch code: the head kernels' 256-workgroup cap (8 waves x 16 rows: a second round beyond 32 768
    rows), the seven chunk buckets and the equal-share rounds of the state-part kernel (beyond 256 blocks of 64 rows), the four
    instantiations and the 256-slab cap of the row-gradient kernel (beyond 8192 rows); and what the entry points refuse."""
    from marl_amd import ops
    q = ops.qtran_plan
    fwd = lambda BT, A: q("fwd", BT, N=2, A=A, AE=64 + A)
    lds5 = ((20 + 25 + 20 + 16) * 256 + 17 * 84 + 80 + 128) * 4
    lds4 = ((16 + 16 + 16 + 16) * 256 + 68 + 64 + 128) * 4
    assert fwd(1, 3) == (5, True, False, 1, lds5, 1, 0, 0) and fwd(1, 0) == (4, False, False, 1, lds4, 1, 0, 0)
    assert fwd(128, 16)[3:6:2] == (1, 1) and fwd(129, 1)[3:6:2] == (2, 1)
    assert fwd(32768, 3)[3:6:2] == (256, 1) and fwd(32769, 3)[3:6:2] == (256, 2) and fwd(65536, 0)[3:6:2] == (256, 2)
    assert fwd(65536 + 5, 0)[3:6:2] == (256, 3)
    assert q("fwd2", 32769, N=1, A=3, AE=67) == (5, True, True, 256, lds5, 2, 0, 0)
    assert q("fwd2", 100, N=1, A=0, AE=64) is None and q("fwd", 100, N=0, A=3, AE=67) is None
    assert q("fwd", 100, N=2, A=17, AE=81) is None and q("bwd", 100, N=2, A=3, AE=66) is None
    b = q("bwd", 32769, N=2, A=3, AE=67)
    assert (b.FT, b.hot, b.grid, b.rounds, b.slabs) == (5, True, 256, 2, 256)
    assert b.lds == ((16 + 20 + 25) * 256 + 64 + 8 * 80) * 4
    assert b.lds_agents == ((20 + 20) * 256 + 17 * 84 + 8 * 16 * 84 + 8 * 16 * 68 + 8 * 16) * 4
    b = q("bwd", 17, N=1, A=0, AE=64)
    assert (b.FT, b.hot, b.grid, b.rounds, b.slabs) == (4, False, 1, 1, 1) and b.lds_agents == ((16 + 16) * 256 + 68 + 8 * 16 * 68 * 2 + 128) * 4
    assert q("fwd", 0, N=2, A=3, AE=67) == (0, False, False, 0, 0, 0, 0, 0)          # nothing to launch
    sp = lambda BT, S, n=1: q("state_parts", BT, S=S, nsets=n)
    for S, kct in ((1, 4), (64, 4), (65, 8), (128, 8), (129, 12), (192, 12), (193, 14), (224, 14), (225, 16), (256, 16), (257, 20), (320, 20),
                   (321, 24), (384, 24)):
        for n in (1, 2):
            assert sp(65, S, n) == (kct, n, 2, 64 * (16 * kct + 4) * 4, 1), (S, n)
    assert sp(16384, 4)[2::2] == (256, 1) and sp(16385, 4)[2::2] == (129, 2) and sp(16384 + 64 * 3 + 1, 4, 2)[2::2] == (130, 2)
    assert sp(64 * 513, 4)[2::2] == (171, 3)
    assert sp(10, 0) is None and sp(10, 385) is None and sp(10, 4, 3) is None
    assert q("qmix_tail", 16385, S=322, nsets=2) == (24, 1, 129, 64 * 388 * 4, 2)
    wg = lambda BT, S, AE: q("wgrad_rows", BT, S=S, AE=AE)
    for S, AE, ft, smax in ((4, 64, 4, 224), (224, 80, 5, 224), (228, 64, 4, 384), (384, 65, 5, 384)):
        p = wg(33, S, AE)
        ts = (S + 15) // 16
        assert p == (ft, smax, 4 * ts + 4 * ft + 16 + ft * ft, 2, 32 * (48 * ft + 260 + smax) * 4, 1, 2), (S, AE, p)
    assert wg(8192, 4, 64)[3:] == (256, wg(1, 4, 64).lds, 1, 256) and wg(8193, 4, 64)[3:] == (256, wg(1, 4, 64).lds, 2, 256)
    assert wg(8192 + 32 * 5 + 7, 224, 80)[5:] == (2, 256) and wg(31, 4, 64)[3] == 1 and wg(8160, 4, 64)[3] == 255
    assert wg(10, 322, 74) is None and wg(10, 388, 78) is None and wg(10, 216, 81) is None and wg(10, 2, 64) is None


def test_mlp3_plan_query():
    """marl_mlp3_plan (a host function, no GPU: the planners the four launches of csrc/mlp3_fused.hip and csrc/mlp3_x6.hip themselves
    decide with; integers stand for the addresses) on QPLEX's action extractors of a 2s3z-sized map - [state 120 | 5 x 11 one-hot],
    10 heads, 3073 rows: the compile-time CF variants, the 6 + 5 stage passes of the kept backward, the stripe arithmetic with its
    empty stripes, the LDS bytes; the bucket steps; and what the entry points refuse."""
    from marl_amd import ops
    from marl_amd._lib import MarlMlp3Weights, MarlSrc

    def weights(three=True, b1=1 << 20):
        w = MarlMlp3Weights()
        w.w1 = w.w3 = w.b3 = 1 << 21
        w.b1 = b1
        if three:
            w.w2 = w.b2 = 1 << 22
        return w

    def src(k0, nhot=0, hot_w=0, ld0=None, p0=4096):
        s = MarlSrc()
        s.p0, s.ld0, s.k0 = p0, (k0 + 3) // 4 * 4 if ld0 is None else ld0, k0
        if nhot:
            s.idx, s.nhot, s.hot_w = 8192, nhot, hot_w
        return s
    q = lambda what, M=3073, G=10, N3=5, s=None, **kw: ops.mlp3_plan(what, kw.pop("w", weights()), s or src(120, 5, 11), M,
                                                                    ops.src_width(s or src(120, 5, 11)), N3, G, Y=1 << 24, **kw)
    f = q("fwd", hsave=1 << 26)
    assert f == (11, 7, 7, 0, 175, True, False, 1, True, 11, 1, 2, 24, 9, 240, (4 * 11 * 256 + 16 * 256 + 4 * 256) * 4 + 4 * 128, False, 0)
    assert q("fwd")._replace(kept=True) == f
    b = q("bwd", hsave=1 << 26)
    assert (b.KC, b.CFT, b.kept, b.KH, b.passes, b.wgpc, b.nst, b.per, b.grid, b.slabs) == (11, 7, True, 6, 2, 2, 48, 2, 480, 48)
    assert b.lds == (16 * 256 + 16 * 64 + max(16 * 6 + 64, 192 + 16) * 68) * 4 + 4 * 128
    r = q("bwd")
    assert (r.kept, r.KH, r.passes, r.wgpc, r.nst, r.per, r.slabs) == (False, 11, 1, 1, 24, 3, 24)
    xf, xb = q("x6_fwd", hsave=1 << 26), q("x6_bwd", hsave=1 << 26)
    assert (xf.KC, xf.CF, xf.CFT, xf.nst, xf.per, xf.lds) == (12, 6, 6, 24, 9, (4 * 6 + 8 + 2) * 768 * 4 + 6 * 128)
    assert (xb.KC, xb.CFT, xb.KH, xb.passes, xb.wgpc, xb.nst, xb.per, xb.slabs) == (12, 6, 4, 3, 2, 48, 2, 48)
    assert q("x6_bwd") is None                                         # the split backward reads kept activations only
    for k0, kc in ((64, 4), (68, 8), (128, 8), (132, 12), (160, 12), (164, 11), (176, 11), (180, 12), (192, 12), (196, 16), (256, 16),
                   (260, 24), (384, 24), (388, 32), (512, 32)):
        assert q("fwd", M=65, G=2, s=src(k0)).KC == kc, k0
    assert q("fwd", M=65, G=2, s=src(516)) is None and q("fwd", M=65, G=2, s=src(508, 1, 5)) is None          # K1 + kpad = 513
    assert q("fwd", M=65, G=2, s=src(509)).KV == 512
    assert q("bwd", M=65, G=2, s=src(196)) is None and q("bwd", M=65, G=2, s=src(196), hsave=1 << 26).KH == 16
    assert q("fwd", M=65, G=2, s=src(120, ld0=121)).CF == 0 and q("fwd", M=65, G=2, s=src(120, p0=4100)).CFT == -1
    wide = lambda s, N3=160, **kw: q("bwd", M=65, G=2, N3=N3, s=s, w=weights(False), grads=weights(False), hsave=1 << 26, **kw)
    w24 = wide(src(322))
    assert (w24.wide, w24.KC, w24.CF, w24.n3t, w24.lds) == (True, 24, 20, 10, 165888 - 128 * 20)
    assert wide(src(322, ld0=323)) is None                           # CF = 0: 165 888 bytes of LDS
    assert wide(src(322), ld=321) is None and wide(src(72), N3=162) is None
    assert q("fwd", w=weights(b1=(1 << 20) + 4)) is None and q("fwd", hsave=(1 << 26) + 4) is None
    assert q("fwd", hsave=1 << 26, hsave_floats=ops.mlp3_save_floats(3073, True, 10) - 1) is None
    assert q("bwd", hsave=1 << 26, ws_bytes=8) is None and q("bwd", hsave=1 << 26, grads=weights(False)) is None
    assert q("fwd", M=0) is None
