"""Propagators: ASM_Prop, CZT_Prop, RSC_Prop (the reference's module paths), Hankel_Prop and Points_Prop."""
from .Hankel_Prop import Hankel_prop  # noqa: F401
from .Points_Prop import Points_prop  # noqa: F401
