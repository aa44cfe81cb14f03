"""MP_HSIR_Net on MI355X: the reference's module surface over hand-written HIP kernels.

Drop-in for the reference's ``net/MP_HSIR.py`` (ZhehuiWu/MP-HSIR): same class name, constructor
signature, ``forward(inp_img (B,C,H,W), task_id)`` contract and ``state_dict`` keys/shapes/dtypes
(658 entries for the natural-scene model, see tests/test_state_dict.py), so the reference's
checkpoints load with ``load_state_dict`` and its train.py/test.py can import this module instead.

What is different is everything underneath.  The modules below only *hold* parameters under the
reference's names; ``forward`` never calls them.  Activations are channels-last (B,H,W,C) in the
compute dtype (fp32 = parity path, bf16 = throughput path) and every PGSSTB block is six launches
of libmphsir (include/mphsir.h):

    win_attn      LN1 + shift + window MSA + proj + spectral-prompt gate   (ref :667-696, :132-152)
    gemm_tok      1x1 qkv conv of the global spectral branch              (ref :98)
    dwconv_gram   depthwise 3x3 + per-head Gram / norms, v out            (ref :98-107)
    spectral_fold normalise, temperature, softmax, fold project_out        (ref :104-113)
    gemm_tok      M_b v + shortcut + DropPath*(sa*gate + .)                (ref :110-113, :715-718)
    gated_mlp     LN2 + fc1 + GELU gate + fc2 + DropPath residual          (ref :719)

The dense 3x3 convs run on the implicit-GEMM kernel conv3x3_tok; pixel (un)shuffle, concatenation and the
two interpolations of TVSP are PyTorch-ROCm glue.  There is no CPU path: without
libmphsir.so, forward raises.

`file:line` citations are relative to the reference repository's net/MP_HSIR.py.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .. import autograd_ops as AG

WINDOW = 8
PROMPT_LEN = 128

# the task sentences fed to the CLIP text encoder (reference :484-506) -- model definition data
_TASK_PROMPTS = {
    "gaussianN": "A hyperspectral image corrupted by Gaussian noise.",
    "complexN": "A hyperspectral image affected by complex noise patterns.",
    "blur": "A hyperspectral image degraded by Gasussian blur.",
    "sr": "A hyperspectral image with reduced spatial resolution.",
    "inpaint": "A hyperspectral image compressed to a certain ratio.",
    "haze": "A hyperspectral image degraded by atmospheric haze.",
    "bandmiss": "A hyperspectral image with missing spectral bands.",
    "cassi": "A hyperspectral image modulated by a coded aperture and compressed into a snapshot measurement.",
}
_TASK_SETS = {6: ("gaussianN", "complexN", "blur", "sr", "inpaint", "bandmiss"),
              7: ("gaussianN", "complexN", "blur", "sr", "inpaint", "haze", "bandmiss"),
              1: ("cassi",)}


def _hidden(dim, factor):
    return int(dim * factor)


_Cache = ops.WeightCache     # per-module cache of kernel-layout weights (see ops.WeightCache / engine.PackPlan)


# --------------------------------------------------------------------------------------------------
# parameter holders (names = reference attribute names; forward is never called on them)
# --------------------------------------------------------------------------------------------------
class GatedMlp(nn.Module):                                                         # ref :66-82
    def __init__(self, in_features, hidden_features):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features * 2)
        self.fc2 = nn.Linear(hidden_features, in_features)


class Spectral_Attention(nn.Module):                                               # ref :85-114
    def __init__(self, dim, num_heads, bias=False):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Conv2d(dim, dim * 3, 1, bias=bias)
        self.qkv_dwconv = nn.Conv2d(dim * 3, dim * 3, 3, padding=1, groups=dim * 3, bias=bias)
        self.project_out = nn.Conv2d(dim, dim, 1, bias=bias)
        self._cache = _Cache()

    def packed(self, dtype):
        ps = [self.qkv.weight, self.qkv_dwconv.weight, self.project_out.weight, self.temperature]
        C = self.project_out.weight.shape[0]

        def build():
            return dict(wqkv=self.qkv.weight.reshape(3 * C, C).to(ops.cdt(dtype)).contiguous(),
                        wqkvT=self.qkv.weight.reshape(3 * C, C).t().to(ops.cdt(dtype)).contiguous(),      # backward: dX = dY W
                        w9=ops.pack_dw(self.qkv_dwconv.weight),
                        wo=self.project_out.weight.reshape(C, C).float().contiguous(),
                        temp=self.temperature.reshape(-1).float().contiguous())
        return self._cache.get(ps, dtype, build)


Attention = Spectral_Attention      # the reference defines the same MDTA math twice more (:289, :394)


class PG_Spectral_Attention(nn.Module):                                            # ref :116-155
    def __init__(self, dim, compress_ratio, num_heads, prompt_len, bias=False):
        super().__init__()
        r = dim // compress_ratio
        self.num_heads = num_heads
        self.linear_down = nn.Linear(dim, r, bias=bias)
        self.linear_up = nn.Linear(r, dim, bias=bias)
        self.linear_prompt = nn.Linear(dim, prompt_len, bias=bias)
        self.prompt_param = nn.Parameter(torch.rand(1, 1, prompt_len, r))
        self.q = nn.Linear(r, r, bias=bias)
        self.kv = nn.Linear(r, 2 * r, bias=bias)
        self.proj = nn.Linear(r, r)


class Spatial_Attention(nn.Module):                                                # ref :158-218
    def __init__(self, dim, window_size, num_heads):
        super().__init__()
        self.num_heads = num_heads
        n = 2 * window_size - 1
        self.relative_position_bias_table = nn.Parameter(torch.zeros(n * n, num_heads))
        t = torch.arange(window_size * window_size)
        ty, tx = t // window_size, t % window_size
        index = (ty[:, None] - ty[None, :] + window_size - 1) * n + (tx[:, None] - tx[None, :] + window_size - 1)
        self.register_buffer("relative_position_index", index)
        self.qkv = nn.Linear(dim, dim * 3, bias=True)
        self.proj = nn.Linear(dim, dim)
        nn.init.trunc_normal_(self.relative_position_bias_table, std=.02)


def shifted_window_mask(H, W, window=WINDOW, shift=WINDOW // 2):
    """(nW,64,64) fp32: 0 where two tokens of a shifted window share a region, -100 otherwise (ref
    calculate_mask :639-660).  Only kept as the `attn_mask` buffer for state_dict parity: the kernel
    derives the mask from coordinates."""
    def reg(n):
        c = torch.arange(n)
        return (c >= n - window).long() + (c >= n - shift).long()
    ids = 3 * reg(H)[:, None] + reg(W)[None, :]
    ids = ids.reshape(H // window, window, W // window, window).permute(0, 2, 1, 3).reshape(-1, window * window)
    return (ids[:, None, :] != ids[:, :, None]).float() * -100.0


class PGSSTB(nn.Module):                                                           # ref :601-723
    def __init__(self, dim, num_heads, input_resolution=(64, 64), window_size=8, shift_size=0, drop_path=0.0,
                 mlp_ratio=4., compress_ratio=8, prompt_len=128, qkv_bias=True, bias=False):
        super().__init__()
        assert window_size == WINDOW and qkv_bias and shift_size in (0, WINDOW // 2)
        self.dim, self.num_heads, self.shift_size = dim, num_heads, shift_size
        self.input_resolution = list(input_resolution)
        self.drop_prob = float(drop_path)
        self.norm1 = nn.LayerNorm(dim)
        self.norm2 = nn.LayerNorm(dim)
        self.mlp = GatedMlp(dim, _hidden(dim, mlp_ratio))
        self.attn = Spatial_Attention(dim, window_size, num_heads)
        self.register_buffer("attn_mask", shifted_window_mask(*self.input_resolution) if shift_size > 0 else None)
        self.gobal_spectral_attn = Spectral_Attention(dim, num_heads, bias)      # (sic) reference spelling
        self.local_spectral_attn = PG_Spectral_Attention(dim, compress_ratio, num_heads, prompt_len, bias)
        self._cache = _Cache()

    def packed(self, dtype):
        a, m, pg = self.attn, self.mlp, self.local_spectral_attn
        ps = [a.qkv.weight, a.qkv.bias, a.proj.weight, a.proj.bias, a.relative_position_bias_table,
              m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias, self.norm1.weight, self.norm1.bias,
              self.norm2.weight, self.norm2.bias] + list(pg.parameters())

        def build():
            W1, b1, W2 = ops.pack_gated_mlp(m.fc1.weight, m.fc1.bias, m.fc2.weight, dtype)
            f = lambda t: t.detach().float().contiguous()
            return dict(
                wqkv=a.qkv.weight.to(ops.cdt(dtype)).contiguous(), bqkv=f(a.qkv.bias),
                wqkvT=a.qkv.weight.t().to(ops.cdt(dtype)).contiguous(),
                wproj=ops.pack_win_proj(a.proj.weight, self.num_heads, dtype), bproj=f(a.proj.bias),
                wprojT=a.proj.weight.t().to(ops.cdt(dtype)).contiguous(),
                rpb=f(a.relative_position_bias_table), W1=W1, b1=b1, W2=W2, b2=f(m.fc2.bias),
                W1T=W1.t().contiguous(), W2T=W2.t().contiguous(),
                ln1=(f(self.norm1.weight), f(self.norm1.bias)), ln2=(f(self.norm2.weight), f(self.norm2.bias)),
                pg={"linear_prompt.weight": f(pg.linear_prompt.weight), "prompt_param": f(pg.prompt_param.reshape(PROMPT_LEN, -1)),
                    "q.weight": f(pg.q.weight), "kv.weight": f(pg.kv.weight), "linear_down.weight": f(pg.linear_down.weight),
                    "proj.weight": f(pg.proj.weight), "proj.bias": f(pg.proj.bias), "linear_up.weight": f(pg.linear_up.weight)})
        return self._cache.get(ps, dtype, build)

    def drop_path_factors(self, B, device):
        """timm DropPath semantics: per-sample Bernoulli(keep)/keep, drawn independently for the two
        residual branches (ref :718-719); None in eval mode or when the rate is 0."""
        if not self.training or self.drop_prob == 0.0:
            return None, None
        pre = self.__dict__.pop("_dp_factors", None)      # drawn for all blocks at once by MP_HSIR_Net.forward
        if pre is not None and pre.shape[1] == B and pre.device == torch.device(device):
            return pre[0], pre[1]
        keep = 1.0 - self.drop_prob
        m = torch.empty((2, B), dtype=torch.float32, device=device).bernoulli_(keep) / keep
        return m[0].contiguous(), m[1].contiguous()

    def forward(self, x, text_prompt=None, res=None, skip=None):
        """x: channels-last (B,H,W,C) in the compute dtype; res: a second residual added to the output by the last launch;
        skip: AG.Skip(holder, first, last) -- the AG.SkipGrad of the enclosing BaseBlock and this block's place in it, see there"""
        k1, k2 = self.drop_path_factors(x.shape[0], x.device)
        return AG.pgsstb(self, x, k1, k2, res, skip)


class BaseBlock(nn.Module):                                                        # ref :727-761
    def __init__(self, dim=96, window_size=8, input_resolution=(64, 64), depth=6, num_head=6, mlp_ratio=2,
                 compress_ratio=8, prompt_len=128, qkv_bias=True, qk_scale=None, drop_path=(), bias=False):
        super().__init__()
        self.blocks = nn.ModuleList(
            PGSSTB(dim, num_head, input_resolution, window_size, 0 if i % 2 == 0 else window_size // 2, drop_path[i],
                   mlp_ratio, compress_ratio, prompt_len, qkv_bias, bias) for i in range(depth))

    def forward(self, x, text_prompt=None):
        y = x
        n = len(self.blocks)
        # (no-grad forward: 512x512 cube 6.99 -> 6.88 ms, batch 16 3.37 -> 3.33 ms; training, round 6: 19.22 -> 19.18 ms for the forward
        # half -- six adds of 5-19 us that the serial trace of the step shows one for one)
        if n == 0:
            for blk in self.blocks:
                y = blk(y)
            return y + x
        # training: the gradient arriving over the skip is handed from the last block's backward to the first block's, whose final launch
        # adds it (AG.SkipGrad) -- otherwise autograd sums the two gradients of x with a launch of its own
        hold = AG.SkipGrad() if (ops.BASE_SKIP_BWD and torch.is_grad_enabled() and x.requires_grad) else None
        for i, blk in enumerate(self.blocks):
            y = blk(y, res=x if i == n - 1 else None,           # the skip `+ x` (ref :760) rides in the last block's gated-MLP launch
                    skip=None if hold is None else AG.Skip(holder=hold, first=i == 0, last=i == n - 1))
        return y


class _LN(nn.Module):
    """holder for LayerNorm(dim, 'WithBias').body.{weight,bias}                     ref :341-370"""

    def __init__(self, dim):
        super().__init__()
        self.body = nn.Module()
        self.body.weight = nn.Parameter(torch.ones(dim))
        self.body.bias = nn.Parameter(torch.zeros(dim))

    def pair(self):
        return self.body.weight.detach().float().contiguous(), self.body.bias.detach().float().contiguous()


class FeedForward(nn.Module):                                                      # ref :251-265 == :374-391
    def __init__(self, dim, ffn_expansion_factor, bias=False):
        super().__init__()
        hid = _hidden(dim, ffn_expansion_factor)
        self.project_in = nn.Conv2d(dim, hid * 2, 1, bias=bias)
        self.dwconv = nn.Conv2d(hid * 2, hid * 2, 3, padding=1, groups=hid * 2, bias=bias)
        self.project_out = nn.Conv2d(hid, dim, 1, bias=bias)
        self._cache = _Cache()

    def packed(self, dtype):
        ps = [self.project_in.weight, self.dwconv.weight, self.project_out.weight]

        def build():
            two_hid, D = self.project_in.weight.shape[:2]
            hid = two_hid // 2
            HP = ops.round_up(hid, 32)
            dev = self.project_in.weight.device
            w_in = torch.zeros((2 * HP, D), dtype=ops.cdt(dtype), device=dev)
            wi = self.project_in.weight.reshape(two_hid, D)
            w_in[:hid], w_in[HP:HP + hid] = wi[:hid].to(ops.cdt(dtype)), wi[hid:].to(ops.cdt(dtype))
            w9 = torch.zeros((9, 2 * HP), dtype=torch.float32, device=dev)
            w9s = ops.pack_dw(self.dwconv.weight)
            w9[:, :hid], w9[:, HP:HP + hid] = w9s[:, :hid], w9s[:, hid:]
            w_out = torch.zeros((D, HP), dtype=ops.cdt(dtype), device=dev)
            w_out[:, :hid] = self.project_out.weight.reshape(D, hid).to(ops.cdt(dtype))
            return dict(w_in=w_in, w9=w9, w_out=w_out, w_inT=w_in.t().contiguous(), w_outT=w_out.t().contiguous())
        return self._cache.get(ps, dtype, build)


FFN = FeedForward


class CrossAttention(nn.Module):                                                   # ref :220-249
    def __init__(self, dim, num_heads, bias=False):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.kv = nn.Conv2d(dim, dim * 2, 1, bias=bias)
        self.kv_dwconv = nn.Conv2d(dim * 2, dim * 2, 3, padding=1, groups=dim * 2, bias=bias)
        self.q = nn.Conv2d(dim, dim, 1, bias=bias)
        self.q_dwconv = nn.Conv2d(dim, dim, 3, padding=1, groups=dim, bias=bias)
        self.project_out = nn.Conv2d(dim, dim, 1, bias=bias)
        self._cache = _Cache()

    def packed(self, dtype):
        ps = [self.kv.weight, self.kv_dwconv.weight, self.q.weight, self.q_dwconv.weight, self.project_out.weight, self.temperature]
        D = self.q.weight.shape[0]

        def build():
            return dict(wq=self.q.weight.reshape(D, D).to(ops.cdt(dtype)).contiguous(),
                        wkv=self.kv.weight.reshape(2 * D, D).to(ops.cdt(dtype)).contiguous(),
                        wqT=self.q.weight.reshape(D, D).t().to(ops.cdt(dtype)).contiguous(),
                        wkvT=self.kv.weight.reshape(2 * D, D).t().to(ops.cdt(dtype)).contiguous(),
                        w9=torch.cat([ops.pack_dw(self.q_dwconv.weight), ops.pack_dw(self.kv_dwconv.weight)], 1).contiguous(),
                        wo=self.project_out.weight.reshape(D, D).float().contiguous(),
                        temp=self.temperature.reshape(-1).float().contiguous())
        return self._cache.get(ps, dtype, build)


class CrossTransformer(nn.Module):                                                 # ref :267-287
    def __init__(self, dim, num_heads, ffn_expansion_factor, bias=False, LayerNorm_type="WithBias", cross_residual=True):
        super().__init__()
        assert LayerNorm_type == "WithBias" and cross_residual
        self.norm11, self.norm12 = _LN(dim), _LN(dim)
        self.attn = CrossAttention(dim, num_heads, bias)
        self.norm2 = _LN(dim)
        self.ffn = FFN(dim, ffn_expansion_factor, bias)


class TransformerBlock(nn.Module):                                                 # ref :466-479
    def __init__(self, dim, num_heads, ffn_expansion_factor, bias=False, LayerNorm_type="WithBias"):
        super().__init__()
        assert LayerNorm_type == "WithBias"
        self.norm1 = _LN(dim)
        self.attn = Attention(dim, num_heads, bias)
        self.norm2 = _LN(dim)
        self.ffn = FeedForward(dim, ffn_expansion_factor, bias)


def surrogate_clip_prompt(task_classes, seed=2024):
    """Seeded stand-in for the CLIP ViT-B/32 text embeddings (T,512): for benchmarks and tests on machines without the
    OpenAI `clip` package / weights.  A model built on it is NOT interchangeable with reference checkpoints."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn((task_classes, 512), generator=g)
    return v / v.norm(dim=-1, keepdim=True) * 8.0


class Text_Prompt(nn.Module):                                                      # ref :481-535
    def __init__(self, task_classes=7, clip_prompt=None):
        super().__init__()
        if task_classes not in _TASK_SETS:
            raise ValueError("task_classes must be 6 or 7")
        self.task_text_prompts = [_TASK_PROMPTS[k] for k in _TASK_SETS[task_classes]]
        self.task_classes = task_classes
        self.clip_source = "injected"
        if isinstance(clip_prompt, str):
            if clip_prompt != "surrogate":
                raise ValueError("clip_prompt must be a (T,512) tensor, None (encode with OpenAI clip) or 'surrogate'")
            clip_prompt, self.clip_source = surrogate_clip_prompt(task_classes), "surrogate"
        elif clip_prompt is None:
            clip_prompt, self.clip_source = self._encode_with_clip(), "clip ViT-B/32"
        assert tuple(clip_prompt.shape) == (task_classes, 512), clip_prompt.shape
        self.clip_prompt = clip_prompt.detach().float()      # plain attribute, not in state_dict
        self._on_device = {}                                  # device copies (no host->device copy inside a captured step)

    def _encode_with_clip(self):
        """the reference's construction-time text encoding (:512-515).  Without the `clip` package this RAISES: silently
        substituting other embeddings would make reference checkpoints evaluate wrongly (the table is not in the
        state_dict).  Pass clip_prompt=<(T,512) tensor> or, for benchmarks/tests, clip_prompt="surrogate"."""
        try:
            import clip  # OpenAI CLIP, as the reference uses it
        except ImportError as e:
            raise RuntimeError(
                "MP_HSIR_Net needs the CLIP ViT-B/32 text embeddings of its task sentences and the OpenAI `clip` package is "
                "not installed.  Pass clip_prompt=<tensor (task_classes,512)> (e.g. saved from a machine that has it, or "
                "read from a checkpoint written by this package), or clip_prompt='surrogate' to opt into a seeded stand-in "
                "(benchmarks / tests only: not interchangeable with reference checkpoints).") from e
        model, _ = clip.load("ViT-B/32", device="cpu")
        with torch.no_grad():
            return model.encode_text(clip.tokenize(self.task_text_prompts)).float()

    def forward(self, x, de_class=None):
        T = self.task_classes
        table = self._on_device.get(x.device)
        if table is None:
            table = self._on_device[x.device] = self.clip_prompt.to(x.device)
        if de_class.dim() > 1:
            w = ops.task_weights(de_class.contiguous(), T)      # training path: mean of one-hots (:519-523)
        else:
            w = F.one_hot(de_class, T)                           # test path: int64 one-hot (:525)
        clip = AG.mix_rows(w, table)                             # (w.unsqueeze(-1) * table).mean(1)  (:527)
        return clip, w

    def get_clip_prompt(self):
        return self.clip_prompt


class TVSP(nn.Module):                                                             # ref :538-583
    def __init__(self, task_classes=6, prompt_size=64, prompt_dim=96, out_dim=96, clip_prompts=None):
        super().__init__()
        self.task_classes, self.prompt_size, self.prompt_dim = task_classes, prompt_size, prompt_dim
        self.text_linear = nn.Linear(512, prompt_dim)         # in the state_dict, unused in forward (Q3)
        self.visual_prompt = nn.Parameter(torch.randn(1, prompt_dim, prompt_size, prompt_size))
        self.clip_linear = nn.Linear(512, prompt_dim)         # likewise
        self.text_prompt_learnable = nn.Parameter(torch.randn(1, task_classes, prompt_dim, 1, 1))
        self.cross_transformer = CrossTransformer(prompt_dim, 2, 2.66, False, "WithBias")
        self.conv_last = nn.Conv2d(prompt_dim, out_dim, 3, padding=1, bias=False)
        self._cache = _Cache()

    def packed(self, dtype):
        """vis1: the one visual prompt map as tokens (ps*ps, D) in the compute dtype (a pure layout change of a parameter: under the engine's
        PackPlan it rides in the per-step weight gather instead of two launches per forward)"""
        ps, D = self.prompt_size, self.prompt_dim
        return self._cache.get([self.visual_prompt], dtype,
                               lambda: dict(vis1=self.visual_prompt[0].permute(1, 2, 0).to(ops.cdt(dtype)).contiguous().reshape(ps * ps, D),
                                            vis1_f32=self.visual_prompt[0].permute(1, 2, 0).float().contiguous().reshape(ps * ps, D)))

    def forward(self, x, clip_prompt=None, prompt_weights=None, out=None):
        """x: channels-last (B,H,W,D) (only its shape is used, as in the reference).  out: see AG.conv3x3."""
        return AG.tvsp(self, x, clip_prompt, prompt_weights, out)


class PromptFusion(nn.Module):                                                     # ref :587-599
    def __init__(self, dim=96, out_dim=48, head=6, ffn_expansion_factor=2.66, bias=False):
        super().__init__()
        self.transformer = TransformerBlock(dim, head, ffn_expansion_factor, bias, "WithBias")
        self.conv = nn.Conv2d(dim, out_dim, 1, bias=bias)

    def forward(self, x, prompt, out=None, joined=None):
        return AG.prompt_fusion(self, x, prompt, out, joined)


class OverlapPatchEmbed(nn.Module):                                                # ref :454-463
    def __init__(self, in_c=3, embed_dim=48, bias=False):
        super().__init__()
        self.proj = nn.Conv2d(in_c, embed_dim, 3, padding=1, bias=bias)


class Downsample(nn.Module):                                                       # ref :432-440
    def __init__(self, n_feat):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(n_feat, n_feat // 2, 3, padding=1, bias=False), nn.PixelUnshuffle(2))


class Upsample(nn.Module):                                                         # ref :442-450
    def __init__(self, n_feat):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(n_feat, n_feat * 2, 3, padding=1, bias=False), nn.PixelShuffle(2))


class MP_HSIR_Net(nn.Module):                                                      # ref :763-844
    def __init__(self, in_channel=31, out_channel=31, dim=64, num_blocks=[2, 4, 6], window_size=[8, 8, 8],
                 task_classes=6, num_refinement_blocks=4, heads=[2, 4, 8], ffn_expansion_factor=2.66, bias=False,
                 clip_prompt=None, compute_dtype=None):
        super().__init__()
        assert list(window_size) == [8, 8, 8], "the kernels are built for 8x8 windows (the only shipped setting)"
        nb = list(num_blocks)
        self.patch_embed = OverlapPatchEmbed(in_channel, dim)
        dpr = [x.item() for x in torch.linspace(0, 0.1, sum(nb))]
        self.text_prompt = Text_Prompt(task_classes=task_classes, clip_prompt=clip_prompt)
        self.clip_prompts = self.text_prompt.get_clip_prompt()
        self.prompt1 = TVSP(task_classes, 64, dim, dim)
        self.prompt2 = TVSP(task_classes, 32, dim * 2, dim * 2)
        self.fusion1 = PromptFusion(dim * 2, dim, 4, 2.66, False)
        self.fusion2 = PromptFusion(dim * 4, dim * 2, 8, 2.66, False)

        def stage(c, res, depth, head, cr, rates):
            return BaseBlock(c, 8, [res, res], depth, head, ffn_expansion_factor, cr, PROMPT_LEN, True, None, rates, bias)
        r1, r2, r3 = dpr[:nb[0]], dpr[nb[0]:nb[0] + nb[1]], dpr[nb[0] + nb[1]:]
        self.encoder_level1 = stage(dim, 64, nb[0], heads[0], 8, r1)
        self.down1_2 = Downsample(dim)
        self.encoder_level2 = stage(dim * 2, 32, nb[1], heads[1], 16, r2)
        self.down2_3 = Downsample(dim * 2)
        self.latent = stage(dim * 4, 16, nb[2], heads[2], 32, r3)
        self.up3_2 = Upsample(dim * 4)
        self.reduce_chan_level2 = nn.Conv2d(dim * 4, dim * 2, 1, bias=bias)
        self.decoder_level2 = stage(dim * 2, 32, nb[1], heads[1], 16, r2)
        self.up2_1 = Upsample(dim * 2)
        self.decoder_level1 = stage(dim * 2, 64, nb[0], heads[0], 8, r1)
        self.refinement = stage(dim * 2, 64, num_refinement_blocks, heads[0], 8, r2)
        self.output = nn.Conv2d(dim * 2, out_channel, 3, padding=1, bias=bias)
        self.prompts = None
        self.compute_dtype = compute_dtype

    def set_compute_dtype(self, dtype):
        """torch.float32 (exact-f32 MFMA, parity path), torch.bfloat16, torch.float16 (the reference's 16-mixed: train it
        through engine.DataParallelEngine, which then turns on dynamic loss scaling), or None = follow autocast."""
        self.compute_dtype = dtype
        return self

    def _dtype(self):
        if self.compute_dtype is not None:
            return self.compute_dtype
        if torch.is_autocast_enabled():
            dt = torch.get_autocast_dtype("cuda") if hasattr(torch, "get_autocast_dtype") else torch.bfloat16
            return dt if dt in (torch.bfloat16, torch.float16) else torch.bfloat16
        return torch.float32

    def _draw_drop_path(self, B, device):
        """timm DropPath factors (Bernoulli(keep)/keep per sample, independent per residual branch) of ALL blocks in two
        launches instead of two per block; each block picks its rows up in drop_path_factors."""
        blks = [m for m in self.modules() if isinstance(m, PGSSTB) and m.drop_prob > 0.0]
        if not self.training or not blks:
            return
        cache = self.__dict__.get("_dp_keep")
        if cache is None or cache.device != torch.device(device) or cache.shape[0] != len(blks):
            cache = self.__dict__["_dp_keep"] = torch.tensor([1.0 - m.drop_prob for m in blks], dtype=torch.float32, device=device)
        keep = cache.reshape(-1, 1, 1).expand(len(blks), 2, B)
        f = torch.bernoulli(keep) / keep
        self.__dict__["_dp_last"] = f          # the factors of the latest forward ((blocks, 2, B); under hipGraph replay: the static buffer)
        for i, m in enumerate(blks):
            m.__dict__["_dp_factors"] = f[i]

    def forward(self, inp_img, task_id=None):
        dt = self._dtype()
        self._draw_drop_path(inp_img.shape[0], inp_img.device)
        clip, w = self.text_prompt(inp_img, task_id)
        x_in = AG.input_head(inp_img, dt)                                          # channels-last (and 32-padded) from here on
        e1 = self.encoder_level1(AG.conv3x3(x_in, self.patch_embed.proj))
        # the prompt branch of each level (ref :827, :835 -- there in program order behind the stages below) is forked where its input
        # exists and joined where the decoder of that level reads it: a parallel branch of the captured graph (inference only,
        # see ops.PROMPT_SIDE)
        fork = ops.PROMPT_SIDE and not torch.is_grad_enabled()
        # the decoder's concatenations [pixel_shuffle(up(.)) | fusion(.)] (ref :838, :843): each producer writes its half of one buffer
        # ... and so do the prompt fusions' inputs [e | prompt] (ref :596): TVSP's last conv writes the right half, e is copied into the left
        C1 = e1.shape[3]
        cat1, pf1 = e1.new_empty((*e1.shape[:3], 2 * C1)), e1.new_empty((*e1.shape[:3], 2 * C1))
        with ops.side_stream(e1, fork, "prompt1", track=False) as br1:
            f1 = self.fusion1(e1, self.prompt1(e1, clip, w, out=pf1[..., C1:]), out=cat1[..., C1:], joined=pf1)
        e2 = self.encoder_level2(AG.pixel_unshuffle2(AG.conv3x3(e1, self.down1_2.body[0])))
        C2 = e2.shape[3]
        cat2, pf2 = e2.new_empty((*e2.shape[:3], 2 * C2)), e2.new_empty((*e2.shape[:3], 2 * C2))
        with ops.side_stream(e2, fork, "prompt2", track=False) as br2:
            f2 = self.fusion2(e2, self.prompt2(e2, clip, w, out=pf2[..., C2:]), out=cat2[..., C2:], joined=pf2)
        lat = self.latent(AG.pixel_unshuffle2(AG.conv3x3(e2, self.down2_3.body[0])))
        up2 = AG.conv3x3(lat, self.up3_2.body[0])
        br2.join(f2)
        d2 = self.decoder_level2(AG.conv1x1(AG.shuffle_join(up2, f2, cat2), self.reduce_chan_level2))
        up1 = AG.conv3x3(d2, self.up2_1.body[0])
        br1.join(f1)
        r = self.refinement(self.decoder_level1(AG.shuffle_join(up1, f1, cat1)))
        return AG.output_head(r, self.output, inp_img)
