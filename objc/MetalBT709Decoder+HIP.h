// The additions the HIP binding makes to MetalBT709Decoder's interface (Renderer/MetalBT709Decoder.h:27-72 itself
// does not change).  A class extension -- imported by objc/MetalBT709Decoder+HIP.m, which is the class's primary
// implementation on an MI355X machine, so the property is synthesized there -- and by the one kind of caller that
// needs it: a renderer that wants several frames in flight.  Every other reference call site compiles and behaves
// as before without importing this header.
#import "MetalBT709Decoder.h"

@interface MetalBT709Decoder ()
// NO (default): a host-memory frame is complete when -decodeBT709:... returns, whatever waitUntilCompleted says, because
// the HIP decode is not part of the caller's MTLCommandBuffer.  YES: with waitUntilCompleted:NO up to MaxBuffersInFlight
// (3, AAPLRenderer.m:34) frames stay in flight on their own HIP streams; the caller invokes -finishHIPFrames before
// [commandBuffer commit].
@property (nonatomic, assign) BOOL hipDeferredCompletion;
// The coalescing submit of the HIP decoder (include/bt709hip_ext.h BT709HIP_OPT_COALESCE / _COALESCE_MAX_AGE_US), for a caller that
// hands this decoder DEVICE-resident frames through its bt709hip handle (hipDecoderHandle) at the reference's one-call-per-frame
// cadence: n = 2..32 frames gathered per launch (0 = off, the default), and the age in microseconds after which a queue is issued
// by the context's next call on any stream (0 = no limit).  Host-memory frames -- this class's own selector -- gain nothing: each
// goes through an in-flight pool slot with a stream of its own and is PCIe-bound.  Set before -setupMetal or at any time after.
@property (nonatomic, assign) int hipCoalesceFrames;
@property (nonatomic, assign) int hipCoalesceMaxAgeMicroseconds;
// The format of the intermediate the FUSED rescales of the HIP decoder filter (bt709hip_decode_scaled / _decode_half through
// hipDecoderHandle; include/bt709hip_ext.h BT709HIP_OPT_SCALE_INTERMEDIATE), named after the choice AAPLRenderer makes for its
// _resizeTexture (AAPLRenderer.m:143-170): MTLPixelFormatBGRA8Unorm_sRGB (0 is read as that default) or
// MTLPixelFormatRGBA16Float -- linear light at half precision, bit for bit what -decodeBT709: into such a texture followed by
// -renderScaled: gives; a decoder without an alpha channel then writes A = 0xFF.  Set before -setupMetal or at any time after.
@property (nonatomic, assign) MTLPixelFormat hipResizeTexturePixelFormat;
// What the 1:1 decode of a decoder with hasAlphaChannel is blended over, inside the decode kernel (device-resident frames through
// hipDecoderHandle; include/bt709hip_ext.h BT709HIP_OPT_COMPOSITE_OVER): BT709HIPCompositeOverOff (the default),
// BT709HIPCompositeOverDestination -- what the target holds when the kernel runs, the non-opaque MTKView over a pattern image of
// AAPLViewController.m:30-66 -- or an opaque sRGB colour R<<16 | G<<8 | B (its black / white backgrounds: 0 / 0xFFFFFF).  The
// property reads BT709HIPCompositeOverOff until it is set.  Set before -setupMetal or at any time after.
enum { BT709HIPCompositeOverOff = -1, BT709HIPCompositeOverDestination = -2 };  // BT709HIP_OVER_OFF, BT709HIP_OVER_DESTINATION
@property (nonatomic, assign) int hipCompositeOver;
// The same for the FUSED rescales (bt709hip_decode_scaled / _decode_half through hipDecoderHandle; BT709HIP_OPT_SCALED_OVER): the
// alpha clip played view-fit over the app's background, blended inside the rescale kernel.  The same values, held separately from
// hipCompositeOver; reads BT709HIPCompositeOverOff until it is set.
@property (nonatomic, assign) int hipScaledCompositeOver;
// YES: the 1:1 decode of a decoder with hasAlphaChannel writes STRAIGHT alpha -- each pixel's B, G, R divided by its own alpha byte
// inside the decode kernel, the GPU twin of +[BGRAToBT709Converter unpremultiply:] (device-resident frames through
// hipDecoderHandle; include/bt709hip_ext.h BT709HIP_OPT_UNPREMULTIPLY).  NO (the default): the premultiplied colour the frames hold.
// While it is YES the rescales, RGBA16Float targets and a decode under hipCompositeOver are refused.  Set before -setupMetal or at
// any time after.
@property (nonatomic, assign) BOOL hipStraightAlpha;
// The bt709hip_decoder behind this object (NULL before -setupMetal), as a void * so that this header needs no bt709hip.h.
- (void *) hipDecoderHandle;
// Completes every frame still in flight: their pixels are copied into the textures passed with them.  Same thread
// as -decodeBT709:... (the in-flight pool is single-threaded).
- (BOOL) finishHIPFrames;
@end
