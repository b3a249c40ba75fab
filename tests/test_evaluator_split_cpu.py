"""CPU: the host side of the InterCLIP evaluator's fp32_split mode (mixermdm_amd/evaluation.py) -- the precision argument and its refusals, the padded
operand width Kp, the layout of the fp16-plane weight twins, and the head-size refusal, all raised before any GPU call."""
import inspect
import pytest

CFG = {"MODE": "interaction", "INPUT_DIM": 258, "ACTIVATION": "gelu", "DROPOUT": 0.1, "EXTENDED": False, "LATENT_DIM": 256, "FF_SIZE": 512, "NUM_LAYERS": 2,
       "NUM_HEADS": 4}


def test_precision_argument_and_its_refusals():
    from mixermdm_amd.evaluation import InterCLIP, EvaluatorModelWrapper, EvaluatorModelWrapperIndividual, PRECISIONS
    assert PRECISIONS == ("fp32", "fp32_split")
    assert inspect.signature(InterCLIP.__init__).parameters["precision"].default == "fp32"
    for cls in (EvaluatorModelWrapper, EvaluatorModelWrapperIndividual):
        assert inspect.signature(cls.__init__).parameters["precision"].default == "fp32"
    m = InterCLIP(CFG)
    assert m.precision == "fp32" and not m.split and m.k_pad == 528          # the default constructor: the fp32 path and its operand width
    assert InterCLIP(CFG, precision="fp32").k_pad == 528
    s = InterCLIP(CFG, precision="fp32_split")
    assert s.precision == "fp32_split" and s.split
    for bad in ("bf16", "fp32-split", "FP32", None, 2):
        with pytest.raises(ValueError, match="precision .* not recognized"):
            InterCLIP(CFG, precision=bad)
    with pytest.raises(RuntimeError, match="no weights loaded"):
        s.encode_text({"tokens_text": [[1, 2]]})


def test_operand_width_is_a_multiple_of_32_in_split_mode():
    from mixermdm_amd.evaluation import InterCLIP, embed_k_pad
    from mixermdm_amd import ops
    assert (embed_k_pad(2, "fp32_split"), embed_k_pad(1, "fp32_split")) == (544, 288)
    assert (embed_k_pad(2), embed_k_pad(1)) == (528, 272)
    assert (ops.split_k_pad(2), ops.split_k_pad(1)) == (544, 288)
    assert InterCLIP(CFG, precision="fp32_split").k_pad == 544
    assert InterCLIP(dict(CFG, MODE="individual"), precision="fp32_split").k_pad == 288
    assert InterCLIP(dict(CFG, MODE="individual")).k_pad == 272


def test_weight_twin_shapes_and_plane_strides():
    from mixermdm_amd.evaluation import interclip_split_twins, interclip_shapes, split_twin_layout
    for cfg, kp in ((CFG, 544), (dict(CFG, MODE="individual", LATENT_DIM=128, NUM_HEADS=2, FF_SIZE=96), 288)):
        D, F, L = cfg["LATENT_DIM"], cfg["FF_SIZE"], cfg["NUM_LAYERS"]
        tw = interclip_split_twins(cfg)
        shapes = interclip_shapes(cfg)
        # a twin for every GEMM weight of both encoders and nothing else: embed, 4 per layer of L motion and 8 text layers, the two output Linears
        gemm = {k for k, s in shapes.items() if len(s) == 2 and k not in ("motion_encoder.query_token", "token_embedding.weight", "positional_embedding")}
        assert set(tw) == gemm and len(tw) == 1 + 4 * (L + 8) + 2
        for k, t in tw.items():
            N, K = shapes[k]
            if k == "motion_encoder.embed_motion.weight":
                K = kp                                                   # zero-padded to Kp
            assert t["shape"] == (2, N, K) and t["plane_stride"] == N * K and K % 32 == 0, k
        assert tw["motion_encoder.embed_motion.weight"]["packed"] is False          # 544 and 288 are no multiples of 64: plain planes
        assert tw["out.weight"]["packed"] is True and tw["motion_encoder.out.weight"]["packed"] is True
        for i in range(8):
            assert tw[f"textTransEncoder.layers.{i}.linear2.weight"]["packed"] is (F % 64 == 0)
        # one storage order per layer: fragment order only when every matrix of the layer is covered
        for i in range(L):
            assert {tw[f"motion_encoder.transformer.layers.{i}.{k}"]["packed"] for k in
                    ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "linear1.weight", "linear2.weight")} == {D % 64 == 0 and F % 64 == 0}
    assert split_twin_layout(512, 544) == {"shape": (2, 512, 544), "plane_stride": 512 * 544, "packed": False}
    with pytest.raises(ValueError, match="K % 32 == 0"):
        split_twin_layout(512, 528)


def test_head_size_refusal_names_the_head_size():
    from mixermdm_amd.evaluation import InterCLIP
    for D, H, hs in ((256, 8, 32), (768, 8, 96), (512, 2, 256)):
        cfg = dict(CFG, LATENT_DIM=D, NUM_HEADS=H)
        InterCLIP(cfg)                                                   # the fp32 mode takes it (its own checks come at the call)
        with pytest.raises(ValueError, match=f"head size {hs}"):
            InterCLIP(cfg, precision="fp32_split")
    for D, H in ((128, 2), (256, 2), (512, 4), (1024, 8)):
        InterCLIP(dict(CFG, LATENT_DIM=D, NUM_HEADS=H), precision="fp32_split")
    with pytest.raises(ValueError, match="multiples of 32"):
        InterCLIP(dict(CFG, FF_SIZE=100), precision="fp32_split")
