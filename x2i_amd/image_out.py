"""The image back end of a sampling call on the HIP path: packed latents in, uint8 pixels on the host out, files written behind the
caller's back (abi/backend/x2i_image_out.h, image_out_binding.py, AutoencoderKL.decode_to_uint8).

  back = ImageBackEnd(vae, device)            # a ring of pinned host buffers with their device twins
  writer = ImageWriter()                      # one background thread: Pillow encodes while the next batch samples
  ticket = back.submit(latents, 1024, 1024)   # enqueues kernel, decoder, kernel, ONE device-to-host copy of 3 bytes per pixel, an event
  writer.put(ticket, ["a.jpg", "b.jpg"])      # the thread waits on the event, saves, gives the slot back
  writer.flush()                              # at the end: joins, re-raises what the thread met

What leaves the device is what is saved: uint8 [B, H, W, 3], bit for bit VaeImageProcessor.postprocess's pixels, so Image.fromarray(a).save(path)
writes the bytes the path without the back end writes.  Nothing here synchronises the device but Ticket.arrays, which waits on its own event.
"""
import queue
import threading

import torch


class Ticket:
    """One submit: B images of H x W pixels on their way into a slot's pinned buffer.  arrays() waits for them; release() gives the slot
    back to the ring, after which the arrays are no longer the caller's (a context manager does both: `with ticket as arrays:`)."""

    def __init__(self, back, slot, B, H, W):
        self._back, self._slot, self.shape = back, slot, (B, H, W)
        self.released = False

    def arrays(self):
        """[H, W, 3] uint8 numpy views of the pinned buffer, one per image, valid until release()"""
        if self.released:
            raise RuntimeError("x2i_amd ImageBackEnd: this ticket was released; its slot may hold another batch")
        self._slot.event.synchronize()
        B, H, W = self.shape
        host = self._slot.host.numpy()[:B * H * W * 3].reshape(B, H, W, 3)
        return [host[i] for i in range(B)]

    def release(self):
        if not self.released:
            self.released = True
            self._back._release(self._slot)

    def __enter__(self):
        return self.arrays()

    def __exit__(self, *exc):
        self.release()
        return False


class _Slot:
    def __init__(self):
        self.nbytes, self.host, self.dev, self.event, self.busy = 0, None, None, None, False


class ImageBackEnd:
    """vae: an x2i_amd.vae.AutoencoderKL on `device`; slots: how many batches may be between submit and release at once (2: one being
    saved, one being computed).  A slot's buffers grow to the largest batch it has served."""

    def __init__(self, vae, device, slots=2):
        if slots < 1:
            raise ValueError("x2i_amd ImageBackEnd: slots=%d must be at least 1" % slots)
        self.vae, self.device = vae, torch.device(device)
        self._slots = [_Slot() for _ in range(slots)]
        self._free = threading.Condition()
        self._next = 0
        self.regrown = 0        # allocations so far (a test's and a bench's view of the ring)

    def image_size(self, height, width):
        """(H, W) of the decoded image for the pipeline's height, width: 2 * (height // vae_scale_factor) latent rows, doubled per up block"""
        n = len(self.vae.config.block_out_channels)
        return 2 * (int(height) // 2 ** n) * 2 ** (n - 1), 2 * (int(width) // 2 ** n) * 2 ** (n - 1)

    def _take(self, timeout):
        """the next slot in ring order, once its ticket was released (the writer thread's doing, as a rule)"""
        with self._free:
            slot = self._slots[self._next]
            if not self._free.wait_for(lambda: not slot.busy, timeout):
                raise RuntimeError("x2i_amd ImageBackEnd: every slot holds a ticket that was not released (slots=%d); release one, or "
                                   "hand the tickets to an ImageWriter" % len(self._slots))
            slot.busy = True
            self._next = (self._next + 1) % len(self._slots)
            return slot

    def _release(self, slot):
        with self._free:
            slot.busy = False
            self._free.notify_all()

    def submit(self, packed_latents, height, width, timeout=None):
        """Enqueue decode_to_uint8 of packed latents [B, (h / 2)(w / 2), 4 C] into a slot's device buffer, one asynchronous copy into its
        pinned twin and an event, all on the current stream; returns the Ticket.  Blocks (up to `timeout` seconds, None: for ever) only
        while the slot whose turn it is holds an unreleased ticket.
        Call it on ONE stream for the life of the back end.  A slot's buffers are torch allocations of the stream that was current when they
        were made, and a regrown slot drops the old pair without record_stream: the allocator may hand that memory out again as soon as
        the allocating stream's work is enqueued.  The wait on the slot's last event orders a submit behind the copy that used the slot
        before, and nothing more."""
        B = packed_latents.shape[0]
        H, W = self.image_size(height, width)
        nbytes = B * H * W * 3
        slot = self._take(timeout)
        try:
            if slot.event is None:
                slot.event = torch.cuda.Event()
            else:
                torch.cuda.current_stream(self.device).wait_event(slot.event)   # behind the slot's last copy (no cost on the one stream)
            if slot.nbytes < nbytes:
                slot.host = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
                slot.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
                slot.nbytes = nbytes
                self.regrown += 1
            self.vae.decode_to_uint8(packed_latents, height, width, out=slot.dev)
            slot.host[:nbytes].copy_(slot.dev[:nbytes], non_blocking=True)
            slot.event.record(torch.cuda.current_stream(self.device))
        except BaseException:
            self._release(slot)
            raise
        return Ticket(self, slot, B, H, W)


class ImageWriter:
    """One background thread that saves the images of (ticket, paths) pairs with Pillow -- Image.fromarray(a).save(path), which releases
    the interpreter lock while it encodes -- and releases each ticket.  The thread touches the GPU through the ticket's event wait alone.
    After a failure it saves nothing more: it releases the tickets still queued without waiting for them, put() refuses, and flush()
    raises the first exception."""

    def __init__(self):
        self._q = queue.Queue()
        self._error = None
        self._thread = threading.Thread(target=self._run, name="x2i-image-writer", daemon=True)
        self._thread.start()

    def _run(self):
        from PIL import Image
        while True:
            item = self._q.get()
            try:
                if item is None:
                    return
                ticket, paths = item
                try:
                    if self._error is None:
                        arrays = ticket.arrays()
                        if len(arrays) != len(paths):
                            raise ValueError("x2i_amd ImageWriter: %d images for %d paths" % (len(arrays), len(paths)))
                        for a, path in zip(arrays, paths):
                            Image.fromarray(a).save(path)
                except BaseException as e:      # kept for flush(); the thread lives on to release what is queued
                    if self._error is None:
                        self._error = e
                finally:
                    ticket.release()
            finally:
                self._q.task_done()

    @property
    def failed(self):
        return self._error is not None

    def put(self, ticket, paths):
        if self._error is not None:
            ticket.release()
            raise RuntimeError("x2i_amd ImageWriter: an earlier image could not be saved (%r); flush() raises it" % (self._error,))
        if not self._thread.is_alive():
            ticket.release()
            raise RuntimeError("x2i_amd ImageWriter: closed")
        self._q.put((ticket, list(paths)))

    def flush(self):
        """wait until everything put so far is saved; raise the first exception the thread met (once)"""
        self._q.join()
        e, self._error = self._error, None
        if e is not None:
            raise e

    def close(self):
        """flush, then end the thread"""
        try:
            self.flush()
        finally:
            if self._thread.is_alive():
                self._q.put(None)
                self._thread.join()
