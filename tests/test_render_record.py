"""contact_sheet and save_gif (roborugby_amd/render.py): what turns render_batch's frames into something to look at.  Host only."""
import numpy as np
import pytest

from roborugby_amd import render


def _frames(m, h, w):
    f = np.zeros((m, h, w, 3), np.uint8)
    f[:] = (np.arange(m, dtype=np.uint8) * 20 + 10)[:, None, None, None]
    return f


@pytest.mark.parametrize("as_torch", [False, True], ids=["numpy", "torch"])
def test_contact_sheet_shapes_and_padding(as_torch):
    f = _frames(5, 6, 8)
    if as_torch:
        torch = pytest.importorskip("torch")
        f = torch.as_tensor(f)
    sheet = render.contact_sheet(f)                      # 5 frames: 3 columns, 2 rows
    assert tuple(sheet.shape) == (2 + 2 * (6 + 2), 2 + 3 * (8 + 2), 3) and type(sheet) is type(f)
    s = np.asarray(sheet)
    pad = render.COLOR_DASHBOARD_FILL[0]
    for k in range(5):
        y, x = 2 + (k // 3) * 8, 2 + (k % 3) * 10
        assert (s[y:y + 6, x:x + 8] == 20 * k + 10).all()
        assert (s[y - 2:y, x - 2:x + 10] == pad).all() and (s[y - 2:y + 8, x - 2:x] == pad).all()   # the margins above and left of it
    assert (s[10:18, 22:32] == pad).all()                # the sixth tile has no frame
    assert (s[-2:] == pad).all() and (s[:, -2:] == pad).all()
    wide = np.asarray(render.contact_sheet(f, cols=5, pad=0))
    assert wide.shape == (6, 40, 3) and all((wide[:, 8 * k:8 * k + 8] == 20 * k + 10).all() for k in range(5))
    tall = np.asarray(render.contact_sheet(f, cols=1, pad=1))
    assert tall.shape == (1 + 5 * 7, 10, 3)
    with pytest.raises(ValueError):
        render.contact_sheet(f[..., :2])


def test_save_gif_writes_every_frame(tmp_path):
    from PIL import Image
    sheets = [render.contact_sheet(_frames(4, 6, 8) + k) for k in range(3)]
    path = render.save_gif(str(tmp_path / "clip.gif"), sheets, fps=25)
    with Image.open(path) as im:
        assert im.format == "GIF" and im.n_frames == 3 and im.size == (sheets[0].shape[1], sheets[0].shape[0])
        assert im.info["duration"] == 40
        im.seek(2)
        assert np.array_equal(np.asarray(im.convert("RGB")), sheets[2])   # 6 grey levels: the palette holds them exactly
    with pytest.raises(ValueError):
        render.save_gif(str(tmp_path / "none.gif"), [])
