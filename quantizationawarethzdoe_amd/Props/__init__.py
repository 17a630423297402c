"""Propagators: ASM_Prop, CZT_Prop, RSC_Prop (the reference's module paths) and Hankel_Prop."""
from .Hankel_Prop import Hankel_prop  # noqa: F401
