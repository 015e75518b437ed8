"""The reduced patch-14 models (DINOv2's patch geometry; head_dim stays 64) that the patch-14 and LayerScale tests share."""
import dataclasses

from vit_amd import synth

TINY14 = synth.ModelConfig(img_size=28, patch_size=14, num_classes=10, embed_dim=128, depth=2, num_heads=2, hidden_dim=256)    # T = 5
SMALL14 = synth.ModelConfig(img_size=56, patch_size=14, num_classes=100, embed_dim=192, depth=3, num_heads=3, hidden_dim=768)  # T = 17
ODD14 = dataclasses.replace(SMALL14, img_size=42)   # T = 10: 9 patches, img_size % 4 == 2
B14 = synth.ModelConfig(patch_size=14)              # ViT-B/14 at 224, full depth: T = 257
CONFIGS14 = {"tiny14": TINY14, "small14": SMALL14, "odd14": ODD14, "b14": B14}
assert (TINY14.tokens, SMALL14.tokens, ODD14.tokens, B14.tokens) == (5, 17, 10, 257)
