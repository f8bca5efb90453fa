from .FMN import FMN, CLB_quad_form, DeviceMatrix  # noqa: F401
