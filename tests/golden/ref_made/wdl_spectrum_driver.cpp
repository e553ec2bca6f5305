// wdl_spectrum_driver.cpp -- the block loop of Audio::synthesize_spectrum (Audio/AudioSynthesis.cpp:230-263) around the reference's own
// WDL_Resampler, for make_wdl_spectrum.py.  Compiled there together with the reference's WDL/resample.cpp into a temporary directory; nothing
// built from it is kept.  The table is ONE row of `wavelength` frames that every channel reads from its own channel_frame_jump on; the
// frequency is given per OUTPUT FRAME and read at the frame a block starts on, as the method reads its Function.
#include <cstdint>

#include "WDL/resample.h"

extern "C" {

// Returns the number of blocks of channel 0 (every channel runs the same loop); wanted[b] is what ResamplePrepare asked for in block b and
// delivered[b] what ResampleOut returned (the first cap of each are stored).
int64_t wdl_spectrum( const float * table, int wavelength, double fundamental, int num_channels, int out_frames, int granularity, const float * freq,
	float * out, int32_t * wanted_out, int32_t * delivered_out, int64_t cap )
	{
	int64_t blocks0 = 0;
	for( int channel = 0; channel < num_channels; ++channel )
		{
		float * o = out + size_t( channel ) * out_frames;
		WDL_Resampler rs;
		rs.SetMode( true, 1, true );

		const int channel_frame_jump = ( float( channel ) / num_channels ) * wavelength;

		int64_t blocks = 0;
		int out_frames_generated = 0;
		int phase_frame = 0;
		while( out_frames_generated < out_frames )
			{
			const double in_freq_c = fundamental;
			const double out_freq_c = freq[out_frames_generated];

			rs.SetRates( out_freq_c, in_freq_c );
			WDL_ResampleSample * rsinbuf = nullptr;
			const int wdl_wanted = rs.ResamplePrepare( granularity, 1, &rsinbuf );

			for( int j = 0; j < wdl_wanted; ++j ) rsinbuf[j] = table[( phase_frame + j + channel_frame_jump ) % wavelength];

			const int delivered = rs.ResampleOut( o + out_frames_generated, wdl_wanted, out_frames - out_frames_generated, 1 );
			if( channel == 0 && blocks < cap ) { wanted_out[blocks] = wdl_wanted; delivered_out[blocks] = delivered; }
			out_frames_generated += delivered;
			phase_frame = ( phase_frame + wdl_wanted ) % wavelength;
			++blocks;
			if( blocks > ( int64_t( 1 ) << 24 ) ) return -1;
			}
		if( channel == 0 ) blocks0 = blocks;
		}
	return blocks0;
	}

}
