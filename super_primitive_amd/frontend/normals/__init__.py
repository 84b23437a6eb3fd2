"""Normal integration (the reference's ``frontend/normals`` package; only ``normals_integration`` is rebuilt, the normals network stays out of scope)."""
