"""One convolution layer of the VAE against expected bits that do not depend on the order of summation (pytest -m gpu), through the diagnostics
entry s2v_diag_vae_conv_run on the cases and input families of oracle/vae_conv_cases.py.

The entry runs the product's own functions on a real handle: the capacity call, set_layout's ring clearing, one launch_* producer from the
test's source, run_conv / run_conv_down with their cache copies and kernel choice, launch_to_ncfhw where conv_out did not run as the direct kernel.
Weights go in through s2v_vae_load_weight (conv_w_repack_k and the 256-row weight padding are the product's) and are reloaded between the weight
sets of family G.  The whole-decode bars of test_gpu_vae.py and test_gpu_vae_encode*.py (fp32 1e-3, bf16 rel-L2 1.7e-2 .. 3e-2) accept a wrong tap
in one K tile, a cache frame in the wrong slot, a stride-2 origin at (0, 0) or a stale ring; tests/test_vae_conv_exact_cpu.py plants each of them
into a torch emulation and shows which case fails.  Here

  * family S: operand in {-1, 0, 1}, weights +-1, integer bias and residual; max|y| <= 256 (bf16) / 2048 (fp16) / < 2^24 (fp32) asserted on the
    CPU before the launch; the fp32 CPU convolution is the exact reference;
  * family G: one-hot weight rows (+-1, +-2, +-1/2) over arbitrary finite bit patterns -- every tap, channels 0 and 63 of every K tile; the centre
    tap on every channel returns the operand (the producers, element for element), the corner taps return ring and cache cells -- and the mirror
    with single operand cells against arbitrary weights;
  * both epilogues (EPI_BIAS; EPI_BIAS_ADD with the residual aliasing the output, as run_resnet calls it), bitwise; no element is excluded;
  * dense outputs start as NaN between 256 guard rows of a sentinel that must survive; the [C][Ftot][H][W] tile keeps NaN in the frames the call
    does not own; the operand buffer is filled with a pattern before the first call of a cache or ring sequence.

Every case names its kernel and asserts it: the 16-bit MFMA kernels through s2v_diag_gemm_plan at this device's CU count, launch_gemm's other
branches (gemm_f32m, the generic kernel) and the direct kernel on what the entry reports -- gemm_plan covers the 16-bit launch only; the entry's
"gemm_f32m" restates launch_gemm_simple's condition (fp32 and gemm_f32m_ok) beside it, it is not read back from the launch.  Each test prints
`MEASURED vae_conv_exact <case> kernel=<name> compared=<n> bitwise` (profiles/r20_vae_conv_exact.txt).

FINDING.  None: on the MI355X (256 CUs) all 35 cases returned the expected bits on gemm_bf16_pp64, gemm_bf16_stag (bf16 and fp16), gemm_f32m, the
generic kernel and conv_out_direct_k at KB = 1, 2 and 4, in every family, with the guards intact and the foreign frames of the tile untouched (105.8 M
elements compared). That includes what was least certain beforehand: subnormal operands and biases come through the 16-bit and the fp32 MFMA and the
generic kernel unflushed (family G forces an eighth of its uniform bit patterns subnormal, and biases are arbitrary bits too, so that subnormal
outputs are expected and compared; conv_out's three bias columns drew no tiny value, so the direct kernel saw subnormal operands but no subnormal
output was expected of it), a product that overflows (+-2 times a value of the largest binade) arrives as the infinity of its sign, the cache holds
the right two frames after the F >= 2 copy, the two-copy F = 1 branch and a first batch of one frame, the stride-2 form reads interior cell (1, 1) at
output (0, 0) and the zero ring at the last row and column, and the ring of a 5 x 7 window is zero after an 8 x 10 one left the fill pattern's
successors there. The row clamp of a_row_base is NOT among the things checked to bits here: the rows it protects are discarded by the epilogue, a
missing clamp is an out-of-bounds read (the CPU file's emulation catches it by its bounds check). No product code changed. The upsampler has no mirror
case (an upsampled cell is a 2 x 2 block: an output would see several terms); its scatter side is read back through the centre tap. Dense outputs have
guard rows but no guard columns: run_conv fixes ldc = cout."""
import ctypes

import pytest
import torch

from oracle import vae_conv_cases as vc
from oracle.norm_cases import Guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_P, _I32, _I64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64


class Device:
    """run_case's backend on the GPU: handles of the diagnostics build, one per configuration, kept for the module"""

    def __init__(self, s2v):
        self.L, self.D = s2v._lib, s2v._lib.diag_lib()
        self.cfg_t = s2v.vae.VaeConfigC
        D = self.D
        D.s2v_diag_gemm_plan.argtypes = [_I32] * 6 + [_I64, ctypes.POINTER(_I32)]
        for fn in (D.s2v_vae_create, D.s2v_vae_enc_create):
            fn.argtypes = [ctypes.POINTER(self.cfg_t), ctypes.POINTER(_P)]
        D.s2v_vae_load_weight.argtypes = [_P, ctypes.c_char_p, _P, ctypes.POINTER(_I64), _I32, _I32, _P]
        D.s2v_vae_destroy.argtypes, D.s2v_vae_destroy.restype = [_P], None
        D.s2v_diag_vae_conv_info.argtypes = [_P, _I32, ctypes.POINTER(_I32)]
        D.s2v_diag_vae_conv_prepare.argtypes = [_P, _I32, _I32, _I32]
        D.s2v_diag_vae_conv_run.argtypes = [_P, ctypes.POINTER(_I32), _P, _P, _P, ctypes.POINTER(_I32), _P]
        self.handles = {}

    def close(self):
        torch.cuda.synchronize()
        for h, _ in self.handles.values():
            self.D.s2v_vae_destroy(h)
        self.handles = {}

    def ok(self, rc):
        assert rc == 0, self.D.s2v_last_error()

    def handle(self, case):
        """(handle, index of the case's layer in for_each_conv order), the layer held to the case's cin, cout, kt and level"""
        hd = case.handle
        key = hd.key() + (case.layer,)
        if key not in self.handles:
            c = self.cfg_t()
            c.latent_channels, c.out_channels, c.num_blocks = hd.cz, 3, len(hd.blocks)
            for i, ch in enumerate(hd.blocks):
                c.block_out_channels[i] = ch
            c.layers_per_block, c.norm_num_groups, c.temporal_compression_ratio = 1, 1, hd.tcr
            c.sample_height, c.sample_width = 64, 64
            c.dtype, c.force_simple = self.L.DTYPE_OF[vc.STORE[hd.dt]], int(hd.simple)
            c.scaling_factor, c.norm_eps = 1.0, 1e-6
            h = _P()
            self.ok((self.D.s2v_vae_enc_create if hd.kind == "enc" else self.D.s2v_vae_create)(ctypes.byref(c), ctypes.byref(h)))
            info = (_I32 * 5)()
            self.ok(self.D.s2v_diag_vae_conv_info(h, 0, info))
            n = info[4]
            layers = []
            for i in range(n):
                self.ok(self.D.s2v_diag_vae_conv_info(h, i, info))
                layers.append(tuple(info[:4]))
            index = {"first": 0, "last": n - 1}.get(case.layer)
            if index is None:
                index = next(i for i, l in enumerate(layers) if l[2] == 1)
            self.handles[key] = (h, index)
            assert layers[index] == (case.cin, case.cout, case.kt, case.level), f"{case.name}: layer {index} is (cin, cout, kt, level) = {layers[index]}"
        h, index = self.handles[key]
        self.ok(self.D.s2v_diag_vae_conv_prepare(h, *case.capacity()))
        return h, index

    def load(self, case, w5, bias):
        h, _ = self.handle(case)
        self.keep = [w5.to(DEV).contiguous(), bias.to(DEV).contiguous()]
        dtype = self.L.DTYPE_OF[vc.STORE[case.dt]]
        for t, suffix in zip(self.keep, (".weight", ".bias")):
            shape = (_I64 * t.ndim)(*t.shape)
            self.ok(self.D.s2v_vae_load_weight(h, (case.weight_name() + suffix).encode(), t.data_ptr(), shape, t.ndim, dtype, self.L.stream_ptr()))
        torch.cuda.synchronize()

    def step(self, case, step, src, resid, shape):
        h, index = self.handle(case)
        dt = vc.STORE[case.dt]
        es = 4 if dt == torch.float32 else 2
        out = Guarded(shape[0], shape[1], shape[1], dt, resid, DEV, guard=vc.gc.GUARD)  # 256 guard rows, the slack of the product's dense buffers; EPI_BIAS_ADD: the residual IS the output buffer (run_resnet: resid == out)
        srcd = src.to(DEV).contiguous()
        p = (_I32 * 24)()
        p[0], p[1], p[2], p[3], p[4], p[5], p[6] = index, step.F, step.H, step.W, int(step.first), step.epi, step.prod
        if step.img:
            p[7], p[8], p[9], p[10], p[11], p[12] = step.img
        if step.tile:
            p[13], p[14], p[15] = 1, step.tile[0], step.tile[1]
        if step.fill:
            p[16], p[17] = es // 2, vc.FILL[es]
        p[18] = int(step.stride2)
        info = (_I32 * 8)()
        body = _P(out.body_ptr())
        self.ok(self.D.s2v_diag_vae_conv_run(h, p, srcd.data_ptr(), body if resid is not None else None, body, info, self.L.stream_ptr()))
        torch.cuda.synchronize()
        return out.body().cpu(), out.guards_intact(), tuple(info[:6])


@pytest.fixture(scope="module")
def device(s2v):
    d = Device(s2v)
    yield d
    d.close()


@pytest.mark.parametrize("name", [c.name for c in vc.CASES])
def test_vae_convolution_returns_the_exact_bits(device, name):
    case = vc.BY_NAME[name]
    vc.assert_plans(case, device.D, torch.cuda.get_device_properties(0).multi_processor_count)
    compared, kernels = vc.run_case(case, device)
    print(f"\nMEASURED vae_conv_exact {name} kernel={'+'.join(kernels)} compared={compared} bitwise")
