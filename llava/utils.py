"""disable_torch_init of the reference's eval scripts: skip the default initialisation of torch.nn.Linear / LayerNorm (the weights are
loaded right after).  The product's modules initialise their own tensors (halva_amd/llama.py), so this only affects plain torch modules."""
import torch


def disable_torch_init():
    torch.nn.Linear.reset_parameters = lambda self: None
    torch.nn.LayerNorm.reset_parameters = lambda self: None
