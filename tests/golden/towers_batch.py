"""Per-sample variant of the fake image tower of towers.py, for fixtures in which the samples of ONE batch differ in whether their
image was dropped (the conditioning dropout of get_batch_input): the draw of sample i depends on its index and on whether THAT
sample's image is all zero, so a wrong dropout mask shows in the tokens.  Pure harness code; no reference source."""
import torch


def image_tokens(index, is_zero, tokens, dim, seed):
    """The tokens sample `index` gets for a real image (is_zero False) or an all-zero one (True)."""
    g = torch.Generator().manual_seed(seed + 2 * index + int(not is_zero))
    return torch.randn(tokens, dim, generator=g)


class PerSampleImageTower(torch.nn.Module):
    """model.embedder: (b, 3, h, w) -> (b, tokens, dim).  Reads the image on the host (one synchronisation per call): a test
    harness, like towers.FakeImageTower."""

    def __init__(self, tokens, dim, seed):
        super().__init__()
        self.tokens, self.dim, self.seed = tokens, dim, seed

    def forward(self, img):
        zero = (img.detach().abs().flatten(1).sum(1) == 0).tolist()
        out = torch.stack([image_tokens(i, z, self.tokens, self.dim, self.seed) for i, z in enumerate(zero)])
        return out.to(img.device)
