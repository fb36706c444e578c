from .simple import SimpleStrategy
from .simple_limit import SimpleLimitStrategy

__all__ = ["SimpleStrategy", "SimpleLimitStrategy"]
