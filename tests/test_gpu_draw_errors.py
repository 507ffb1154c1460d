"""The error texts of checks that sit behind shared helpers of the C ABI layer: the texture validation of
pt_sample_counts_derive / pt_sample_counts_pool (one helper that takes the entry point's name) and the SVGF draws'
input planes (one helper per sampler name). Each text is asserted whole: a host reads it through pt_last_error.

Every call here is refused before anything is launched. The checks come after the library's own "pt_init() has not
been called" check, so they need an initialised library, which needs a device: hence the gpu mark.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 8, 8
PT_ERR_MISSING_TEXTURE, PT_ERR_ARG, PT_ERR_STATE = -4, -6, -9


def _refused(call, code, text):
    from ptsvgf import _lib

    with pytest.raises(_lib.PtError) as e:
        call()
    assert e.value.code == code, e.value
    assert _lib.pt().pt_last_error().decode() == text


@pytest.fixture()
def planes(gpu):
    """Two W x H textures, one of another width, and a texture buffer."""
    gl = gpu
    a, b, wide = gl.getTextureRGB32F(W, H), gl.getTextureRGB32F(W, H), gl.getTextureRGB32F(W + 1, H)
    buf = gl.texture_buffer(np.zeros((4, 3), np.float32))
    yield gl, a, b, wide, buf
    for t in (a, b, wide, buf):
        gl.destroy_texture(t)


@pytest.mark.parametrize("fn", ["pt_sample_counts_derive", "pt_sample_counts_pool"])
def test_sample_counts_texture_checks(planes, fn):
    gl, a, b, wide, buf = planes
    p0, p1 = gl.device_ptr(a), gl.device_ptr(b)  # any two device planes: no call here gets as far as reading them

    def call(motion, nd):
        if fn == "pt_sample_counts_derive":
            return lambda: gl.sample_counts_derive(p0, motion, nd, 0.5, 0.1, 4, p1)
        return lambda: gl.sample_counts_pool(0, 0, 4, 0, motion, nd, 0.5, 2.0, 1.0, 0, 0.1, 4, p0, p1)

    missing = fn + " needs the 2-D textures gMotion and gNormalAndLinearZ"
    _refused(call(0, b), PT_ERR_MISSING_TEXTURE, missing)  # no such handle
    _refused(call(a, buf), PT_ERR_MISSING_TEXTURE, missing)  # not a 2-D texture
    _refused(call(a, wide), PT_ERR_ARG, fn + ": textures of different sizes")
    gl.set_band(W, H, 2, 6, 0, H)
    try:
        _refused(call(a, b), PT_ERR_STATE, fn + ": not under a pt_set_band partition")
    finally:
        gl.set_band(W, H, 0, H, 0, H)


def test_svgf_input_plane_checks(planes):
    """svgf_modulate.frag's first input, by the name the pass samples it under."""
    gl, a, b, wide, buf = planes
    p = gl.RenderPass(gl.getShaderProgram("svgf_modulate.frag", "vert.vert"), W, H)
    p.colorAttachments = [a]
    p.bindData()
    try:
        p.set_texture_uniform(gl.GL_TEXTURE_BUFFER, buf, "gAlbedo")
        _refused(p.draw, PT_ERR_MISSING_TEXTURE, "pass needs 2-D texture 'gAlbedo'")
        p.set_texture_uniform(gl.GL_TEXTURE_2D, wide, "gAlbedo")
        _refused(p.draw, PT_ERR_ARG, "texture 'gAlbedo' size differs from the pass size")
        p.set_texture_uniform(gl.GL_TEXTURE_2D, b, "gAlbedo")
        p.set_texture_uniform(gl.GL_TEXTURE_BUFFER, buf, "gEmission")
        _refused(p.draw, PT_ERR_MISSING_TEXTURE, "pass needs 2-D texture 'gEmission'")
    finally:
        p.destroy()
