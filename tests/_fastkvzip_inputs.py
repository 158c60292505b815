"""Seeded inputs of the FastKVzip tests and the specs of their fixtures (tests/golden/fastkvzip_*.npz, oracle/gen_golden_fastkvzip.py).
Kernel inputs are rounded to the dtype they are stored in, so the float64 oracle and the kernel read the same numbers.  Gates are
initialised so that every term matters (k_base and b ~ N(0, 0.5), norm weights uniform in 0.5 .. 1.5): the reference's zeros and ones make
the gate degenerate."""
import numpy as np

TILE = 128          # tokens per workgroup of the matrix-core kernel
EPS = 1e-6          # Qwen3RMSNorm's default, read from the module by the press

# ---- flow fixtures: the REAL FastKVzipPress on the tiny float32 Llama (hidden 24, 2 kv heads, 2 query heads each, 2 layers) ------------------
# seed: where the generator's search starts (it skips seeds whose selection boundary is closer than 10 x the contract bound to a tie; the
# seed it kept is recorded in the fixture, and so are the ids and the gates: no test replays the generator's random numbers)
FLOW = {
    "fastkvzip_flow_120_r02": dict(tokens=120, compression_ratio=0.2, layerwise=False, seed=21),
    "fastkvzip_flow_120_r08": dict(tokens=120, compression_ratio=0.8, layerwise=False, seed=22),
    "fastkvzip_flow_56_r02": dict(tokens=56, compression_ratio=0.2, layerwise=False, seed=23),
    "fastkvzip_flow_56_r08": dict(tokens=56, compression_ratio=0.8, layerwise=False, seed=24),
    "fastkvzip_flow_120_layerwise": dict(tokens=120, compression_ratio=0.5, layerwise=True, seed=25),
    "fastkvzip_flow_40_allones": dict(tokens=40, compression_ratio=0.2, layerwise=False, seed=26),     # window 0: every score is 1.0
}
GATE_KEYS = ("q_proj.weight", "q_proj.bias", "k_proj.weight", "q_norm.weight", "k_norm.weight", "k_base", "b")


def flow_ids(seed, tokens):
    """int64 [1, tokens]; ids 3 .. 63 (0 pad, 1 bos, 2 eos stay out)"""
    return np.random.RandomState(2000 + seed).randint(3, 64, size=(1, tokens)).astype(np.int64)


def make_gates(gate_cls, seed, llama_config, dtype=None, sink=16, output_dim=16):
    """seeded gates of a model's geometry from the given class (the reference's in the generator, this package's in the tests)"""
    import torch

    dtype = dtype or torch.float32
    torch.manual_seed(seed)
    nhead = llama_config.num_key_value_heads
    gates = []
    for l in range(llama_config.num_hidden_layers):
        g = gate_cls(l, llama_config.hidden_size, nhead, llama_config.num_attention_heads // nhead, dtype, output_dim, sink)
        with torch.no_grad():
            g.q_proj.bias.copy_((0.5 * (2 * torch.rand(g.q_proj.bias.shape) - 1)).to(dtype))
            g.q_norm.weight.copy_(0.5 + torch.rand(output_dim))
            g.k_norm.weight.copy_(0.5 + torch.rand(output_dim))
            g.k_base.copy_(0.5 * torch.randn(g.k_base.shape))
            g.b.copy_((0.5 * torch.randn(g.b.shape)).to(dtype))
        gates.append(g.eval())
    return gates


def gates_state(gates):
    """{"gate<l>/<key>": array} of a list of gates (bf16 / f16 as float32 arrays)"""
    return {f"gate{l}/{k}": v.detach().float().cpu().numpy() for l, g in enumerate(gates) for k, v in g.state_dict().items()}


def load_gates(g, llama_config, dtype=None):
    """this package's FastKVzipGate per layer holding the weights a fixture recorded (strict)"""
    import torch

    from kvpress_amd.presses.fastkvzip_press import FastKVzipGate

    dtype = dtype or torch.float32
    nhead = llama_config.num_key_value_heads
    gates = []
    for l in range(llama_config.num_hidden_layers):
        sd = {k[len(f"gate{l}/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith(f"gate{l}/")}
        gate = FastKVzipGate(l, llama_config.hidden_size, nhead, llama_config.num_attention_heads // nhead, dtype, sd["q_norm.weight"].shape[0],
                             sd["k_base"].shape[2])
        gate.load_state_dict({k: v.to(gate.state_dict()[k].dtype) for k, v in sd.items()}, strict=True)
        gates.append(gate.eval())
    return gates


def gate_arrays(state, layer):
    """(wq, bq, wk, b [Hkv,G], gq, gk, kb [Hkv,J,D]) of one layer of a fixture / gates_state dict, as the oracle takes them"""
    g = {k: np.asarray(state[f"gate{layer}/{k}"]) for k in GATE_KEYS}
    return (g["q_proj.weight"], g["q_proj.bias"], g["k_proj.weight"], g["b"][:, 0], g["q_norm.weight"], g["k_norm.weight"], g["k_base"][:, 0])


# ---- kernel inputs ------------------------------------------------------------------------------------------------------------------------
def round_to(x, dtype):
    """float32 array holding x rounded to "f32" / "f16" / "bf16" """
    import torch

    from _inputs import torch_dtype

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch_dtype(dtype)).float().numpy()


# (dtype, B, S, K, Hkv, G, J[, D = 16]).  Matrix-core path: S in {1, T - 1, T, T + 1, 2 T + 3}, K in {32, 96 (the K tail), 4096 (S <= T + 5)},
# geometries (8, 4) = 640 columns (one head group of 640 weight rows), (8, 8) (two head groups of 4 heads = 576 rows), (2, 2), (1, 1) and
# (8, 3) = even G + 1 (one group of 512 rows); J in {16, 4, 0}; B = 2.  The dispatch picks 512 or 640 rows a workgroup by shape;
# tests/test_gpu_fastkvzip.py also forces each.  Generic path: float32, K no multiple of 32, other D, G > 8, J > 16.
T = TILE
MFMA_CASES = [
    ("bf16", 1, 1, 32, 8, 4, 16), ("f16", 1, T - 1, 96, 8, 4, 16), ("bf16", 1, T, 4096, 8, 4, 16), ("bf16", 1, T + 1, 4096, 8, 8, 16),
    ("f16", 2, 2 * T + 3, 96, 8, 8, 16), ("bf16", 1, 2 * T + 3, 32, 2, 2, 16), ("f16", 1, T + 1, 96, 1, 1, 16), ("bf16", 2, T - 1, 32, 8, 3, 16),
    ("f16", 1, 1, 4096, 8, 3, 16), ("bf16", 1, T + 1, 96, 8, 4, 0), ("f16", 2, T, 32, 2, 2, 4), ("bf16", 2, T + 5, 4096, 2, 2, 4),
    ("bf16", 1, 2 * T + 3, 96, 8, 4, 16), ("f16", 1, T, 4096, 1, 1, 16), ("bf16", 1, T + 1, 32, 8, 8, 4),
]
GENERIC_CASES = [
    ("f32", 1, 17, 24, 2, 2, 16), ("f32", 2, 65, 32, 8, 4, 4), ("f32", 1, 5, 4096, 2, 2, 16), ("bf16", 1, 33, 24, 2, 2, 16), ("f16", 2, 9, 40, 2, 3, 5, 8),
    ("f32", 1, 3, 96, 1, 1, 0, 64), ("bf16", 1, 7, 64, 2, 9, 17),        # G > 8 and J > 16 at an otherwise matrix-core shape
]
REFERENCE_ERROR_FIXTURE = "fastkvzip_cases"      # per 16-bit case: the reference gate's own max abs error in that dtype against float64


def case_id(case):
    return "-".join(map(str, case))


def case_seed(case):
    return sum(int(v) for v in case[1:]) + (7 if case[0] == "f16" else 0)


def score_case(case, seed=None):
    """hidden states [B,S,K] ~ N(0,1) and one gate: projections initialised as nn.Linear is (uniform in +-1/sqrt(K)), bq uniform in +-0.5,
    b and k_base ~ N(0, 0.5), norm weights uniform in 0.5 .. 1.5"""
    dtype, B, S, K, Hkv, G, J = case[:7]
    D = case[7] if len(case) > 7 else 16
    rs = np.random.RandomState(case_seed(case) if seed is None else seed)
    a = 1.0 / np.sqrt(K)
    return dict(x=round_to(rs.standard_normal((B, S, K)), dtype), wq=round_to(rs.uniform(-a, a, size=(Hkv * G * D, K)), dtype),
                bq=round_to(0.5 * rs.uniform(-1, 1, size=Hkv * G * D), dtype), wk=round_to(rs.uniform(-a, a, size=(Hkv * D, K)), dtype),
                b=round_to(0.5 * rs.standard_normal((Hkv, G)), dtype), gq=rs.uniform(0.5, 1.5, size=D).astype(np.float32),
                gk=rs.uniform(0.5, 1.5, size=D).astype(np.float32), kb=(0.5 * rs.standard_normal((Hkv, J, D))).astype(np.float32),
                eps=EPS, dtype=dtype, B=B, S=S, K=K, Hkv=Hkv, G=G, J=J, D=D)


def exact_case(case):
    """integer x, Wq, Wk in +-{1, 2} and small integer bq: every product and every partial sum of a projection is exact in float32 (and the
    inputs in bf16 / f16), so NO summation order can change a projected value and a lost or doubled element moves it by at least 1.  The
    rest of the gate is score_case's."""
    s = score_case(case, seed=77 + sum(int(v) for v in case[1:]))
    rs = np.random.RandomState(99 + sum(int(v) for v in case[1:]))
    for name in ("x", "wq", "wk"):
        s[name] = (rs.randint(1, 3, size=s[name].shape) * rs.choice([-1.0, 1.0], size=s[name].shape)).astype(np.float32)
    s["bq"] = rs.randint(-3, 4, size=s["bq"].shape).astype(np.float32)
    return s


def oracle_args(s):
    return tuple(s[n] for n in ("x", "wq", "bq", "wk", "b", "gq", "gk", "kb", "eps"))
