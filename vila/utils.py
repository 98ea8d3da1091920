"""reference vila/utils.py:111-117 (the only piece the VILA evaluation scripts import): disable_torch_init, the llava twin's."""
from llava.utils import disable_torch_init  # noqa: F401
