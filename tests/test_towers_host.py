"""Host algebra of the CLIP text tower (lgd_amd/clip.py) and of the OWL-ViT towers (lgd_amd/owlvit.py) vs transformers'
own modules, on the CPU: what tests/test_sam_host.py is for SAM.  The kernel calls are redirected to the torch restatement
of tests/ops_emul.py with fp32 storage, so this checks the weight loading (fused q/k/v, the names each checkpoint uses),
the shared pre-LN layer of lgd_amd/vit.py, the patch unfolding with the position table as the GEMM's residual, the class
token, the merge and the pooling — not the HIP kernels (tests/test_clip_gpu.py and tests/test_owl_detect_gpu.py do that
on the MI355X).  The heads kernel of OWL-ViT has no restatement and stays with the GPU test.

Every gate is 3 x the value first measured (in the comment next to it), on the towers as they stood before they moved
onto lgd_amd/vit.py; the error is fp32 summation order only."""
import pytest
import torch

import lgd_amd  # noqa: F401
import ops_emul
import owl_detect_cases as cases
from lgd_amd import clip, owlvit, vit

transformers = pytest.importorskip("transformers")


def relerr(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def gate(what, value, limit):
    print(f"{what}: {value:.3e} (limit {limit:.1e})")
    assert value < limit, what


@pytest.fixture()
def emulated_ops(monkeypatch):
    ops_emul.install(monkeypatch, clip, owlvit, vit)


# measured, worst of the eight cases, relative to the tensor maximum: last_hidden_state, worst hidden_states entry,
# pooler_output, text_embeds
CLIP_MEASURED = (3.426e-7, 3.267e-7, 3.556e-7, 4.411e-7)
CLIP_GATES = tuple(3 * m for m in CLIP_MEASURED)


@pytest.mark.parametrize("eos", [2, 5])
@pytest.mark.parametrize("projection", [False, True])
@pytest.mark.parametrize("hidden_act", ["quick_gelu", "gelu"])
def test_clip_text_tower_vs_transformers(emulated_ops, hidden_act, projection, eos):
    """2 layers, 64 wide, 4 heads, 16 positions, B = 2.  eos_token_id 2 is the legacy convention (pooled row at
    argmax(input_ids): the rows end in the highest id, then zero padding); with eos_token_id 5 the pooled row is the first
    5, which lies below every word id, so that the two conventions pick different rows of the same ids."""
    hf_cfg = transformers.CLIPTextConfig(vocab_size=1000, hidden_size=64, intermediate_size=128, num_hidden_layers=2,
                                         num_attention_heads=4, max_position_embeddings=16, hidden_act=hidden_act,
                                         projection_dim=32, eos_token_id=eos, bos_token_id=998, pad_token_id=0)
    torch.manual_seed(0)
    hf = (transformers.CLIPTextModelWithProjection if projection else transformers.CLIPTextModel)(hf_cfg).float().eval()
    ids = torch.randint(10, 998, (2, 16), generator=torch.Generator().manual_seed(1))
    ids[:, 0] = 998
    for b, n in enumerate((4, 11)):
        ids[b, n], ids[b, n + 1:] = (999, 0) if eos == 2 else (5, 5)
    with torch.no_grad():
        want = hf(input_ids=ids, output_hidden_states=True)
        want_pooled = want.text_embeds if projection else want.pooler_output
    enc = clip.from_hf(hf, "cpu")
    assert enc.cfg.eos_token_id == eos and (enc.text_projection is not None) == projection
    got = enc(ids, output_hidden_states=True)
    assert enc(ids).hidden_states is None
    name = f"clip {hidden_act} projection={projection} eos={eos}"
    gate(f"{name} last_hidden_state", relerr(got.last_hidden_state, want.last_hidden_state), CLIP_GATES[0])
    assert len(got.hidden_states) == len(want.hidden_states) == 3
    gate(f"{name} hidden_states", max(relerr(g, w) for g, w in zip(got.hidden_states, want.hidden_states)), CLIP_GATES[1])
    if projection:                      # transformers' projected module does not return the pooled row itself
        assert got[0] is got.text_embeds and got[1] is got.last_hidden_state
        gate(f"{name} text_embeds", relerr(got.text_embeds, want_pooled), CLIP_GATES[3])
    else:
        assert got[0] is got.last_hidden_state
        gate(f"{name} pooler_output", relerr(got.pooler_output, want_pooled), CLIP_GATES[2])
    assert torch.equal(got.pooler_output, got.last_hidden_state[torch.arange(2), [4, 11]])


# measured, relative to the tensor maximum: image_embeds, text_embeds of the real rows (transformers with its padding
# mask), text_embeds of all rows (transformers without it)
OWL_MEASURED = (8.354e-7, 3.607e-7, 3.607e-7)
OWL_GATES = tuple(3 * m for m in OWL_MEASURED)


def test_owlvit_towers_vs_transformers(emulated_ops):
    """tiny_hf_config: 96^2 image, 36 + 1 tokens, B = 2, Q = 3, query row 4 all zero.  transformers applies the padding
    mask and the detector does not: on the real rows that cannot show (the tower is causal and the pooled row lies before
    the padding), so they are compared with the masked run; the all-zero row is compared with a run of transformers
    without the mask, which is what the detector computes for it, and its query mask is 0."""
    cfg = cases.tiny_hf_config()
    torch.manual_seed(0)
    hf = cases.redraw_weights(transformers.OwlViTForObjectDetection(cfg), seed=3)
    B, Q = 2, 3
    pv, ids = cases.model_inputs(cfg, B, Q, seed=4, zero_rows=(4,))
    with torch.no_grad():
        want = hf(input_ids=ids, pixel_values=pv, attention_mask=(ids > 0).long())
        want_unmasked = hf(input_ids=ids, pixel_values=pv)
    det = owlvit.from_hf(hf, "cpu")
    feats = det.encode_image(pv)
    assert feats.shape == (B * det.P, cfg.vision_config.hidden_size)
    gate("owlvit image_embeds", relerr(feats.reshape(want.image_embeds.shape), want.image_embeds), OWL_GATES[0])
    te, mask = det.encode_queries(ids, B)
    assert te.shape == want.text_embeds.shape and mask.tolist() == [[1, 1, 1], [1, 0, 1]]
    real = mask.bool()
    gate("owlvit text_embeds, real rows", relerr(te[real], want.text_embeds[real]), OWL_GATES[1])
    gate("owlvit text_embeds, all rows", relerr(te, want_unmasked.text_embeds), OWL_GATES[2])
