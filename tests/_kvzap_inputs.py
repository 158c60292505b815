"""Seeded inputs of the KVzap / DMS tests and the specs of their fixtures (tests/golden/kvzap_*.npz, oracle/gen_golden_kvzap.py).
Kernel inputs are rounded to the dtype they are stored in, so the float64 oracle and the kernel read the same numbers."""
import numpy as np

U = 2.0 ** -24     # unit roundoff of float32: the contract is written in it

# ---- the fixtures: the REAL DMSPress(KVzapPress) on the tiny float32 Llama ------------------------------------------------------------------
BATCH, PROMPT_TOKENS, DECODE_TOKENS, WINDOW = 2, 70, 6, 16
FIXTURES = {
    "kvzap_mlp": dict(model_type="mlp", hidden_dim=32, seed=11),
    "kvzap_linear": dict(model_type="linear", hidden_dim=None, seed=12),
}


def fixture_ids(seed):
    """(prompt ids [B, 70], the teacher-forced decoding ids [B, 6]) int64; ids 3 .. 63 (0 pad, 1 bos, 2 eos stay out)"""
    rs = np.random.RandomState(1000 + seed)
    return rs.randint(3, 64, size=(BATCH, PROMPT_TOKENS)).astype(np.int64), rs.randint(3, 64, size=(BATCH, DECODE_TOKENS)).astype(np.int64)


def make_surrogate(config_cls, model_cls, spec, llama_config):
    """a seeded surrogate of the tiny Llama's geometry from the given classes (the reference's in the generator, this package's in the
    tests -- which then load the fixture's weights, so no test depends on replaying the generator's random numbers)"""
    import torch

    torch.manual_seed(spec["seed"])
    cfg = config_cls(input_dim=llama_config.hidden_size, output_dim=llama_config.num_key_value_heads, hidden_dim=spec["hidden_dim"],
                     n_modules=llama_config.num_hidden_layers)
    return model_cls(cfg).eval()


def load_surrogate(spec, g, llama_config):
    """this package's KVzapModel holding the weights the fixture recorded"""
    import torch

    from kvpress_amd.presses.kvzap_press import KVzapConfig, KVzapModel

    model = make_surrogate(KVzapConfig, KVzapModel, spec, llama_config)
    model.load_state_dict({k[len("weight/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("weight/")})
    return model


def layer_weights(g, spec, layer):
    """(w1, b1, w2, b2) of one layer as the fixture holds them (w2 = b2 = None for the linear model)"""
    if spec["hidden_dim"] is None:
        return g[f"weight/layers.{layer}.weight"], g[f"weight/layers.{layer}.bias"], None, None
    return (g[f"weight/layers.{layer}.0.weight"], g[f"weight/layers.{layer}.0.bias"], g[f"weight/layers.{layer}.2.weight"],
            g[f"weight/layers.{layer}.2.bias"])


def bound(K, N):
    """the contract's factor of `scale`: 2 (K + N + 4) u"""
    return 2.0 * (K + N + 4) * U


# ---- kernel inputs ------------------------------------------------------------------------------------------------------------------------
def round_to(x, dtype):
    """float32 array holding x rounded to "f32" / "f16" / "bf16" """
    import torch

    from _inputs import torch_dtype

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(torch_dtype(dtype)).float().numpy()


def score_case(seed, B, S, K, N, Hout, dtype):
    """hidden states [B,S,K] ~ N(0,1) and a surrogate layer initialised as nn.Linear is (uniform in +-1/sqrt(fan_in)), biases made as large
    as the pre-activations' spread so that they matter; N = 0: the linear model"""
    rs = np.random.RandomState(seed)

    def lin(o, i, bias_scale):
        a = 1.0 / np.sqrt(i)
        return round_to(rs.uniform(-a, a, size=(o, i)), dtype), round_to(bias_scale * rs.uniform(-1, 1, size=o), dtype)

    x = round_to(rs.standard_normal((B, S, K)), dtype)
    w1, b1 = lin(N or Hout, K, 0.5)
    w2, b2 = lin(Hout, N, 0.5) if N else (None, None)
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dtype=dtype, B=B, S=S, K=K, N=N, Hout=Hout)


def exact_case(B, S, K, N, Hout, dtype, drop=None):
    """integer data whose every partial sum is exact in float32 (and every product in bf16 / f16): |x| and |W1| in {1, 2}, small integer
    biases, so NO summation order can change a bit and a lost or doubled element moves the sum by at least 1.  linear: both signs, the
    exact sum.  mlp: everything positive, so the pre-activations are >= K and gelu(z) = z to 1e-16; W2 is one-hot (output o reads hidden
    unit pick[o]): out = gelu(integer) + b2."""
    rs = np.random.RandomState(77 + K + N + S)
    sign = (lambda shape: rs.choice([-1.0, 1.0], size=shape)) if N == 0 else (lambda shape: 1.0)
    rows = N or Hout
    x = (rs.randint(1, 3, size=(B, S, K)) * sign((B, S, K))).astype(np.float32)
    w1 = (rs.randint(1, 3, size=(rows, K)) * sign((rows, K))).astype(np.float32)
    b1 = rs.randint(-3, 4, size=rows).astype(np.float32)
    w2 = b2 = pick = None
    if N:
        pick = rs.randint(0, N, size=Hout)
        pick[0], pick[-1] = N - 1, 0          # the tile-boundary hidden units are read
        w2 = np.zeros((Hout, N), np.float32)
        w2[np.arange(Hout), pick] = 1.0
        b2 = rs.randint(-2, 3, size=Hout).astype(np.float32)
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, dtype=dtype, B=B, S=S, K=K, N=N, Hout=Hout, pick=pick)
