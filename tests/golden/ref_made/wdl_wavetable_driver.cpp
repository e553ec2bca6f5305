// wdl_wavetable_driver.cpp -- the block loop of Wavetable::synthesize (Wavetable.cpp:293-330) around the reference's own WDL_Resampler, for
// make_wdl_wavetable.py.  Compiled there together with the reference's WDL/resample.cpp into a temporary directory; nothing built from it
// is kept.  The table is float[ch][slots * W] like the C ABI of include/flanhip.h; the frequency and the table index are given per OUTPUT
// FRAME (freq[frame], index[ch][frame]) and read at the frame a block starts on, as the method reads its Functions.
#include <cmath>
#include <cstdint>
#include <vector>

#include "WDL/resample.h"

extern "C" {

// Returns the number of blocks of channel 0 (every channel runs the same loop); wanted[b] is what ResamplePrepare asked for in block b and
// delivered[b] what ResampleOut returned (the first cap of each are stored).
int64_t wdl_wavetable( const float * table, int num_channels, int slots, int wavelength, float sample_rate, int out_frames, int granularity,
	const float * freq, const float * index, int smooth, float * out, int32_t * wanted_out, int32_t * delivered_out, int64_t cap )
	{
	int64_t blocks0 = 0;
	for( int channel = 0; channel < num_channels; ++channel )
		{
		const float * tab = table + size_t( channel ) * slots * wavelength;
		float * o = out + size_t( channel ) * out_frames;
		WDL_Resampler rs;
		rs.SetMode( true, 1, true );

		int64_t blocks = 0;
		int out_frames_generated = 0;
		int phase_frame = 0;
		while( out_frames_generated < out_frames )
			{
			const double in_freq_c = double( sample_rate ) / wavelength;
			const double out_freq_c = freq[out_frames_generated];
			const float table_index_c = index[size_t( channel ) * out_frames + out_frames_generated];
			const int left_index = std::floor( table_index_c );
			const int right_index = std::ceil( table_index_c );
			const float index_remainder = table_index_c - left_index;

			rs.SetRates( out_freq_c, in_freq_c );
			WDL_ResampleSample * rsinbuf = nullptr;
			const int wdl_wanted = rs.ResamplePrepare( granularity, 1, &rsinbuf );

			for( int j = 0; j < wdl_wanted; ++j )
				{
				const float left_sample = tab[( phase_frame + j ) % wavelength + wavelength * left_index];
				if( smooth )
					{
					const float right_sample = tab[( phase_frame + j ) % wavelength + wavelength * right_index];
					rsinbuf[j] = ( 1.0f - index_remainder ) * left_sample + index_remainder * right_sample;
					}
				else rsinbuf[j] = left_sample;
				}

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
