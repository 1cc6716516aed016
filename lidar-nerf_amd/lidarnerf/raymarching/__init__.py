from .raymarching import (composite_rays, composite_rays_train, composite_rays_train_lidar, march_capacity, march_rays, march_rays_train, morton3D, morton3D_invert,  # noqa: F401
                          near_far_from_aabb, packbits, sph_from_ray)
from .raymarching import (ALIVE_N_STEP0, ALIVE_N_STEP_MAX, alive_compact, alive_max_rounds, alive_n_step,  # noqa: F401
                          lidar_composite_rays, lidar_march_rays)
