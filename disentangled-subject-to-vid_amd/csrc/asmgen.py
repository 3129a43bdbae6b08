"""What the asm generators (gen_attn_q4.py, gen_gemm_g4.py, gen_gemm_g4t.py, gen_gemm_g4f.py) write the same way: register names, the
emitter with its ablation filter, the writers of the .inc and *_regs.h files, and the few instruction groups the GEMM loops share.
Plain functions that return text; schedules, register maps and LDS maps stay in the generators.  build.py hashes this file with each."""
import os


def vr(b, n=1):
    return f"v{b}" if n == 1 else f"v[{b}:{b + n - 1}]"


def ar(b, n=1):
    return f"a{b}" if n == 1 else f"a[{b}:{b + n - 1}]"


def sr(b, n=1):
    return f"s{b}" if n == 1 else f"s[{b}:{b + n - 1}]"


def out_dir(script):
    """where a generator writes: beside itself, or S2V_GEN_OUT (tests/test_host_cpu.py regenerates into a scratch directory)"""
    return os.environ.get("S2V_GEN_OUT") or os.path.dirname(os.path.abspath(script))


def ablations(var):
    """the names in the comma-separated environment variable `var` (G4_ABLATE, Q4_ABLATE, G4T_ABLATE): timing experiments of tools/*_ablate.sh
    and tools/stall_*.py that drop instructions from the finished stream -- results are wrong by construction"""
    return set(filter(None, os.environ.get(var, "").split(",")))


def drops_opcodes(ablate, table):
    """predicate for emitter(): the line's opcode is listed in `table` under a name present in `ablate`"""
    gone = {op for name, ops in table.items() if name in ablate for op in ops}
    return lambda ln: ln.split()[0] in gone


def emitter(drop=None):
    """(lines, emit): emit(*lines) appends every non-empty line that `drop` does not reject"""
    L = []

    def emit(*lines):
        L.extend(ln for ln in lines if ln and not (drop and drop(ln)))

    return L, emit


def write_inc(path, lines):
    """one C string literal per instruction: the file is the template of an asm statement"""
    with open(path, "w") as f:
        for ln in lines:
            f.write('"' + ln + '\\n\\t"\n')


def define_regs(name, cls, base, n=1):
    """#define NAME "{v[a:b]}": an operand constraint that pins a physical register range"""
    return f'#define {name} "{{{cls}{base}}}"\n' if n == 1 else f'#define {name} "{{{cls}[{base}:{base + n - 1}]}}"\n'


def define_clobbers(name, regs, tail=("vcc", "scc", "m0", "memory")):
    return f"#define {name} " + ", ".join(f'"{c}"' for c in list(regs) + list(tail)) + "\n"


# ---- shared by the K loops of gemm_g4 / gemm_g4t / gemm_g4f (128-byte LDS rows, 32-row fragments, eight 4-KiB LDS-DMA pieces per operand)
def frag_read(dst, addr, n):
    """16 bytes of fragment n (0-3 W, 4-7 A) of a k-step: the 32-row block is the immediate, the k-step is in the address register"""
    return f"ds_read_b128 {vr(dst, 4)}, {vr(addr)} offset:{(n & 3) * 4096}"


def ptr_advance(s, step=128):
    """64-bit SGPR pointer += step (an immediate or an SGPR name); 128 bytes = one K-tile"""
    return [f"s_add_u32 s{s}, s{s}, {step}", f"s_addc_u32 s{s + 1}, s{s + 1}, 0"]


def m0_piece(base, off):
    """M0 <- LDS address of a piece: SGPR `base` + off.  The piece's LDS-DMA follows at least one instruction later."""
    return f"s_add_u32 m0, s{base}, {off}"


def lds_dma(voff, ptr):
    """one 4-KiB piece: global -> LDS at M0, 16 bytes per lane from the SGPR pointer pair + the lane's 32-bit offset"""
    return f"global_load_lds_dwordx4 {vr(voff)}, {sr(ptr, 2)}"
